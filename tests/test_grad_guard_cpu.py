"""CPU: the training guard's host side (include/gfv.h gfv_grad_guard_dev / gfv_adam_step_guarded_dev, gfv/guard.py) - the new
entry points are declared, bound and exported, refuse bad arguments before anything touches a device, and the Python owners
refuse a policy that cannot work before they touch a model."""
import ctypes as C
import os
import re

import pytest
import torch

import cases

NEW = ("gfv_grad_guard_workspace_bytes", "gfv_grad_guard_dev", "gfv_adam_step_guarded_dev")


def test_guard_symbols_are_declared_bound_and_exported():
    from gfv import lib
    handle = lib.load()
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    declared = set(re.findall(r"\b(gfv_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in lib.declared_symbols(), name
        assert hasattr(handle, name), name
    assert handle.gfv_abi_version() == lib.ABI_VERSION == 3     # new entry points only
    # the policy / decision bits of the binding are the header's
    enum = re.search(r"enum \{ GFV_GUARD_CLIP = (\d+), GFV_GUARD_SKIP_NONFINITE = (\d+), GFV_GUARD_SKIP_FLAG = (\d+) \}", header)
    assert tuple(int(v) for v in enum.groups()) == (lib.GUARD_CLIP, lib.GUARD_SKIP_NONFINITE, lib.GUARD_SKIP_FLAG)
    ws = handle.gfv_grad_guard_workspace_bytes()
    assert ws >= 16 and ws % 8 == 0


def test_guard_entry_points_reject_bad_arguments_without_a_gpu():
    """Negative return codes, nothing launched: the pointers below are host memory no kernel may ever see."""
    from gfv import lib
    handle = lib.load()
    buf = (C.c_double * 512)()      # 8-byte aligned stand-in for every pointer argument
    a = C.addressof(buf)
    ok = dict(g=a, segs=a, n_seg=1, n_elems=4, hyper=a, guard=a, ws=a)

    def guard(**kw):
        v = dict(ok, **kw)
        return handle.gfv_grad_guard_dev(v["g"], v["segs"], v["n_seg"], v["n_elems"], v["hyper"], v["guard"], v["ws"], None)
    for name in ("g", "segs", "hyper", "guard", "ws"):
        assert guard(**{name: None}) < 0, name
    assert guard(n_seg=0) < 0 and guard(n_seg=-3) < 0          # an empty segment table
    assert guard(n_elems=0) < 0 and guard(n_elems=-1) < 0
    assert guard(ws=a + 4) < 0                                  # the partial sums are doubles

    def adam(p=a, g=a, m=a, v=a, n=4, state=a, hyper=a, rec=a):
        return handle.gfv_adam_step_guarded_dev(p, g, m, v, n, state, hyper, rec, None)
    for name in ("p", "g", "m", "v", "state", "hyper", "rec"):
        assert adam(**{name: None}) < 0, name
    assert adam(n=0) < 0 and adam(n=-5) < 0


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan")])
def test_bad_max_grad_norm_is_a_value_error(bad):
    from gfv.guard import check_policy
    from gfv.optim import Adam
    from gfv.pool_trainer import PoolTrainStep
    from gfv.trainer import TrainStep
    with pytest.raises(ValueError, match="max_grad_norm"):
        check_policy(bad)
    # (the check comes first in every constructor: no model, batch or GPU is needed to be told)
    with pytest.raises(ValueError, match="max_grad_norm"):
        TrainStep(None, None, max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        PoolTrainStep(None, None, use_graph=False, max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        Adam([torch.nn.Parameter(torch.zeros(3))], max_grad_norm=bad)


def test_skip_on_flag_with_a_distributed_step_is_a_value_error():
    from gfv.guard import check_policy
    from gfv.trainer import TrainStep
    check_policy(1.0, skip_on_flag=True, dist_on=False)
    check_policy(None, skip_on_flag=False, dist_on=True)
    with pytest.raises(ValueError, match="rank-local"):
        TrainStep(None, None, distributed=True, skip_on_flag=True)
    with pytest.raises(ValueError, match="rank-local"):
        TrainStep(None, None, world_size=2, skip_on_flag=True)


def test_segments_leave_out_padding_and_skipped_parameters():
    from gfv.engine import GradStore
    from gfv.guard import segments
    names, shapes = ["a", "b", "c", "d", "e"], [(3,), (4, 2), (8,), (5,), (1,)]
    G = GradStore(names, shapes, "cpu", skip=("c",))
    # offsets 0, 4, 12, 20, 28: `a` ends one short of `b` (a gap), `b` runs into the skipped `c`, `d` pads 3, `e` is the tail
    assert segments(G) == [(0, 3), (4, 8), (20, 5), (28, 1)]
    G2 = GradStore(["w", "v"], [(4, 4), (8,)], "cpu")
    assert segments(G2) == [(0, 24)]     # neighbours without a gap are one segment
