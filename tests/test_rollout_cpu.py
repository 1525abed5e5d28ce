"""CPU: the guards of the forward-only rollout (gfv/rollout.py, csrc/rollout.hip) - nothing here touches a GPU."""
import ctypes as C

import pytest
import torch

import cases


def _cpu_model(**kw):
    from FVMmodel.importer import NNmodel
    from gfv.params import default_params
    return NNmodel(default_params(**kw))


def test_rollout_advance_rejects_bad_arguments_before_touching_a_device():
    from gfv import lib as L
    lib = L.load(raw=True)
    assert "gfv_rollout_advance" in L.declared_symbols()
    buf = (C.c_double * 64)()          # host memory stands in for every pointer: a refused call reads none of them
    p = C.cast(buf, C.c_void_p).value
    ok = dict(uvp=p, xb=p, x=p, N=4, cb=p, ce=p, gp=p, nc=1, B=1, losses=p, ws=p, hist=p, K=4, state=p)

    def call(**kw):
        a = {**ok, **kw}
        return lib.gfv_rollout_advance(a["uvp"], a["xb"], a["x"], a["N"], a["cb"], a["ce"], a["gp"], a["nc"], a["B"], a["losses"],
                                       a["ws"], a["hist"], a["K"], a["state"], None)
    for name in ("uvp", "xb", "x", "cb", "ce", "gp", "losses", "ws", "hist", "state"):
        assert call(**{name: None}) == -1, name
    for name in ("N", "nc", "B", "K"):
        assert call(**{name: 0}) == -1, name
        assert call(**{name: -3}) == -1, name
    assert call(xb=p + 4) == -1        # the node state rows are read and written 16 bytes at a time


def test_trans_mlp_forward_only_form_needs_both_saved_tensors_null():
    """gfv_trans_mlp_fwd: fx1 and z are both given (saving form) or both NULL (forward-only form); one of the two is an error,
    found before any launch."""
    from gfv import lib as L
    lib = L.load(raw=True)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    a = L.TransMlp()
    for f in ("x", "res", "img_out", "img_pre", "img_post", "gamma", "beta", "wmax", "out"):
        setattr(a, f, p)
    a.M = 8
    a.fx1, a.z = p, None
    assert lib.gfv_trans_mlp_fwd(C.byref(a), None) == -1
    a.fx1, a.z = None, p
    assert lib.gfv_trans_mlp_fwd(C.byref(a), None) == -1


def test_rollout_refuses_cpu_tensors_like_require_gpu():
    from gfv import functions as GF
    from gfv.rollout import Rollout
    graphs = cases.make_graphs("cavity_mixed_b1")
    with pytest.raises(RuntimeError) as want:
        GF.require_gpu(graphs[0].x)
    with pytest.raises(RuntimeError) as got:
        Rollout(_cpu_model(), graphs, max_steps=4)
    assert str(got.value) == str(want.value)


def test_history_overflow_raises_instead_of_writing_past_it():
    from gfv.rollout import check_room
    check_room(0, 4)
    check_room(3, 4)
    check_room(0, 4, steps=4)
    with pytest.raises(IndexError, match="max_steps=4"):
        check_room(4, 4)
    with pytest.raises(IndexError):
        check_room(2, 4, steps=3)


def test_weight_guard_demands_a_refresh_after_a_parameter_change():
    from gfv.rollout import WeightGuard
    model = _cpu_model()
    g = WeightGuard(model)
    g.check()
    g.check()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.load_state_dict(sd)                       # same values, but the images can no longer be vouched for
    with pytest.raises(RuntimeError, match="refresh_weights"):
        g.check()
    g.refresh()
    g.check()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()                                      # an in-place update of every parameter
    with pytest.raises(RuntimeError, match="refresh_weights"):
        g.check()
    g.refresh()
    with torch.no_grad():
        next(model.parameters()).mul_(1.0)
    with pytest.raises(RuntimeError, match="refresh_weights"):
        g.check()


def test_no_grad_forward_still_refuses_cpu_tensors():
    """The torch.no_grad() branch of NNmodel.forward is the forward-only engine path, not an eager PyTorch fallback."""
    graphs = cases.make_graphs("cavity_mixed_b1")
    graphs[0].norm_uvp, graphs[0].norm_global = True, True
    with torch.no_grad(), pytest.raises(RuntimeError, match="must live on the GPU"):
        _cpu_model()(*graphs)
