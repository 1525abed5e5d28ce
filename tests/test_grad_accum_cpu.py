"""CPU: the host side of gradient accumulation (include/gfv.h gfv_grad_accum_dev / gfv_grad_guard_accum_dev /
gfv_adam_step_accum_dev, gfv/accum.py) - the new entry points are declared, bound and exported, refuse bad arguments before
anything touches a device, and the step objects refuse an `accum_steps` that cannot work before they touch a model."""
import ctypes as C
import os
import re

import pytest

import cases

NEW = ("gfv_grad_accum_dev", "gfv_grad_guard_accum_dev", "gfv_adam_step_accum_dev")


def test_accum_symbols_are_declared_bound_and_exported():
    from gfv import lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in lib.declared_symbols(), name
        assert hasattr(handle, name), name
    assert handle.gfv_abi_version() == lib.ABI_VERSION == 3     # new entry points only


def test_accum_entry_points_reject_bad_arguments_without_a_gpu():
    """Negative return codes, nothing launched: the pointers below are host memory no kernel may ever see."""
    from gfv import lib
    handle = lib.load()
    buf = (C.c_double * 512)()      # 8-byte aligned stand-in for every pointer argument
    a = C.addressof(buf)

    def accum(g=a, acc=a, n=4, B=1, loss=a, rec=a):
        return handle.gfv_grad_accum_dev(g, acc, n, B, loss, rec, None)
    for name in ("g", "acc", "loss", "rec"):
        assert accum(**{name: None}) < 0, name
    assert accum(n=-1) < 0 and accum(n=-(1 << 40)) < 0
    assert accum(B=0) < 0 and accum(B=-2) < 0

    ok = dict(g=a, segs=a, n_seg=1, n_elems=4, hyper=a, guard=a, ws=a, rec=a)

    def guard(**kw):
        v = dict(ok, **kw)
        return handle.gfv_grad_guard_accum_dev(v["g"], v["segs"], v["n_seg"], v["n_elems"], v["hyper"], v["guard"], v["ws"], v["rec"],
                                               None)
    for name in ("g", "segs", "hyper", "guard", "ws", "rec"):
        assert guard(**{name: None}) < 0, name
    assert guard(n_seg=0) < 0 and guard(n_elems=0) < 0 and guard(n_elems=-1) < 0
    assert guard(ws=a + 4) < 0                                  # the partial sums are doubles

    def adam(p=a, g=a, m=a, v=a, n=4, state=a, hyper=a, grd=a, rec=a):
        return handle.gfv_adam_step_accum_dev(p, g, m, v, n, state, hyper, grd, rec, None)
    for name in ("p", "g", "m", "v", "state", "hyper", "rec"):
        assert adam(**{name: None}) < 0, name
        assert adam(grd=None, **{name: None}) < 0, name         # (guard == NULL alone is the unguarded form, not an error)
    assert adam(n=0) < 0 and adam(n=-5) < 0


@pytest.mark.parametrize("bad", [0, -1, 2.5, True])
def test_bad_accum_steps_is_a_value_error(bad):
    from gfv.accum import check_accum_steps
    from gfv.pool_trainer import PoolTrainStep
    from gfv.trainer import TrainStep
    with pytest.raises(ValueError, match="accum_steps"):
        check_accum_steps(bad)
    # (the check sits beside check_policy in the constructors: no model, batch or GPU is needed to be told)
    with pytest.raises(ValueError, match="accum_steps"):
        TrainStep(None, None, accum_steps=bad)
    with pytest.raises(ValueError, match="accum_steps"):
        PoolTrainStep(None, None, accum_steps=bad)
    with pytest.raises(ValueError, match="accum_steps"):
        PoolTrainStep(None, None, use_graph=False, accum_steps=bad)


def test_accumulation_with_a_data_parallel_step_is_a_value_error():
    from gfv.accum import check_accum_steps
    from gfv.pool_trainer import PoolTrainStep
    from gfv.trainer import TrainStep
    assert check_accum_steps(1, dist_on=True) == 1 and check_accum_steps(8) == 8
    with pytest.raises(ValueError, match="weighted exchange"):
        check_accum_steps(2, dist_on=True)
    with pytest.raises(ValueError, match="weighted exchange"):
        TrainStep(None, None, accum_steps=2, distributed=True)
    with pytest.raises(ValueError, match="weighted exchange"):
        TrainStep(None, None, accum_steps=2, world_size=2)
    with pytest.raises(ValueError, match="weighted exchange"):
        PoolTrainStep(None, None, accum_steps=2, distributed=True)
