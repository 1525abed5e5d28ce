"""CPU: the host side of gfv.optim.LBFGS - the strong-Wolfe search on scalars against torch's own search on the same problems,
the constructor's refusals, and the argument checks of the gfv_lbfgs_* entry points (which run before anything touches a
device)."""
import ctypes as C

import pytest
import torch


def _torch_search(f, df, x0, d, t, max_ls=25, tolerance_change=1e-9):
    """torch.optim.lbfgs._strong_wolfe on f along d from x0, in float64."""
    from torch.optim.lbfgs import _strong_wolfe
    x0 = torch.as_tensor(x0, dtype=torch.float64).reshape(-1)
    d = torch.as_tensor(d, dtype=torch.float64).reshape(-1)

    def obj(x, tt, dd):
        p = x + tt * dd
        return float(f(p)), df(p)

    f0, g0 = float(f(x0)), df(x0)
    gtd0 = g0.dot(d)
    f_new, _, t_new, evals = _strong_wolfe(obj, x0, t, d, f0, g0, gtd0, max_ls=max_ls, tolerance_change=tolerance_change)
    return float(f_new), float(t_new), int(evals)


def _our_search(f, df, x0, d, t, max_ls=25, tolerance_change=1e-9):
    from gfv.linesearch import strong_wolfe
    x0 = torch.as_tensor(x0, dtype=torch.float64).reshape(-1)
    d = torch.as_tensor(d, dtype=torch.float64).reshape(-1)
    kept = []

    def phi(tt):
        p = x0 + tt * d
        return float(f(p)), float(df(p).dot(d))

    f_new, t_new, evals = strong_wolfe(phi, t, float(f(x0)), float(df(x0).dot(d)), max_ls=max_ls,
                                       tolerance_change=tolerance_change, d_norm=float(d.abs().max()), keep=kept.append)
    assert all(len(k) <= 2 for k in kept)   # never more than two points to hold on to beside the one being evaluated
    return f_new, t_new, evals


def _quartic_far(p):
    return ((p - 30.0) ** 4).sum() * 1e-3


def _quartic_far_grad(p):
    return 4e-3 * (p - 30.0) ** 3


def _rosenbrock(p):
    return 100 * (p[1] - p[0] ** 2) ** 2 + (1 - p[0]) ** 2


def _rosenbrock_grad(p):
    return torch.stack((-400 * p[0] * (p[1] - p[0] ** 2) - 2 * (1 - p[0]), 200 * (p[1] - p[0] ** 2)))


A = torch.tensor([1.0, 10.0, 100.0, 0.5], dtype=torch.float64)
B = torch.tensor([1.0, -2.0, 3.0, 0.25], dtype=torch.float64)

PROBLEMS = {
    # name: (f, grad, x0, d, t, max_ls)
    "quadratic": (lambda p: (0.5 * p * p).sum() - 3.0 * p.sum(), lambda p: p - 3.0, [0.0], [1.0], 1.0, 25),
    "quadratic_vector": (lambda p: 0.5 * (A * p * p).sum() - (B * p).sum(), lambda p: A * p - B, [0.0, 0.0, 0.0, 0.0],
                         [1.0, -2.0, 3.0, 0.25], 1.0, 25),
    "quartic_far_minimum": (_quartic_far, _quartic_far_grad, [0.0], [1.0], 0.01, 25),       # the bracket has to expand
    "exp_plus_square": (lambda p: (torch.exp(-p) + p * p).sum(), lambda p: -torch.exp(-p) + 2 * p, [0.0], [1.0], 1.0, 25),
    "exp_plus_square_small_step": (lambda p: (torch.exp(-p) + p * p).sum(), lambda p: -torch.exp(-p) + 2 * p, [0.0], [1.0], 1e-3, 25),
    "starts_past_the_minimum": (lambda p: (0.5 * p * p).sum() - 3.0 * p.sum(), lambda p: p - 3.0, [0.0], [1.0], 50.0, 25),  # zoom at once
    "past_the_minimum_vector": (lambda p: 0.5 * (A * p * p).sum() - (B * p).sum(), lambda p: A * p - B, [0.0, 0.0, 0.0, 0.0],
                                [1.0, -2.0, 3.0, 0.25], 4.0, 25),
    "hits_max_ls_expanding": (_quartic_far, _quartic_far_grad, [0.0], [1.0], 1e-6, 4),
    "hits_max_ls_zooming": (_rosenbrock, _rosenbrock_grad, [-1.2, 1.0], [215.6, 88.0], 1.0, 3),   # and returns t = 0
    "max_ls_zero": (lambda p: (0.5 * p * p).sum() - 3.0 * p.sum(), lambda p: p - 3.0, [0.0], [1.0], 1.0, 0),
    "rosenbrock_steepest": (_rosenbrock, _rosenbrock_grad, [-1.2, 1.0], [215.6, 88.0], 1.0, 25),
}


# evaluations each case takes (what makes it the case its name says: the bracket grows over several evaluations, the zoom is
# entered at once, the budget of max_ls + 1 evaluations runs out), and where the step must end up relative to its start
EVALS = {"quadratic": 1, "quadratic_vector": 2, "quartic_far_minimum": 4, "exp_plus_square": 2, "exp_plus_square_small_step": 3,
         "starts_past_the_minimum": 2, "past_the_minimum_vector": 2, "hits_max_ls_expanding": 5, "hits_max_ls_zooming": 4,
         "max_ls_zero": 1, "rosenbrock_steepest": 8}
STEP = {"quartic_far_minimum": lambda t: t > 1.0,            # grew a hundredfold from 0.01
        "starts_past_the_minimum": lambda t: t < 50.0,
        "hits_max_ls_zooming": lambda t: t == 0.0}           # the search hands back the starting point


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_strong_wolfe_returns_torchs_step_count_and_value(name):
    f, df, x0, d, t, max_ls = PROBLEMS[name]
    ft, tt, et = _torch_search(f, df, x0, d, t, max_ls)
    fo, to, eo = _our_search(f, df, x0, d, t, max_ls)
    print(f"{name}: torch t={tt!r} f={ft!r} evals={et}; ours t={to!r} f={fo!r} evals={eo}")
    assert eo == et == EVALS[name]
    assert STEP.get(name, lambda t: True)(to)
    assert abs(to - tt) <= 1e-12 * abs(tt)
    assert abs(fo - ft) <= 1e-12 * abs(ft)


def test_constructor_refusals():
    from gfv.optim import LBFGS
    cpu = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(RuntimeError, match="fp32 parameters on the GPU"):
        LBFGS(cpu)
    with pytest.raises(ValueError, match="parameter groups"):
        LBFGS([{"params": [torch.nn.Parameter(torch.zeros(3))]}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])
    with pytest.raises(ValueError, match="history_size"):
        LBFGS(cpu, history_size=129)
    with pytest.raises(ValueError, match="history_size"):
        LBFGS(cpu, history_size=0)
    with pytest.raises(ValueError, match="line_search_fn"):
        LBFGS(cpu, line_search_fn="armijo")
    # torch's defaults
    import inspect
    ours, theirs = inspect.signature(LBFGS.__init__).parameters, inspect.signature(torch.optim.LBFGS.__init__).parameters
    assert list(ours) == list(theirs)
    assert all(ours[k].default == theirs[k].default for k in ours if k not in ("self", "params"))


def test_lbfgs_entry_points_reject_bad_arguments_without_a_gpu():
    from gfv import lib
    h = lib.load()
    buf = (C.c_double * 64)()                      # host memory: never dereferenced, the checks come first
    a = C.addressof(buf)
    a = a + (-a) % 16
    ok, odd = a, a + 4
    n, slots = 1024, 11
    assert h.gfv_lbfgs_workspace_doubles(slots, n) == 3 * (2 * slots + 1) + 2
    assert h.gfv_lbfgs_workspace_doubles(130, n) == 0 and h.gfv_lbfgs_workspace_doubles(slots, 1023) == 0
    assert h.gfv_lbfgs_workspace_doubles(129, n) > 0 and h.gfv_lbfgs_workspace_doubles(1, n) == 0
    # pair(S, Y, slots, n, state, g, g_prev, d, t, first, stream)
    good = [ok, ok, slots, n, ok, ok, ok, ok, 1.0, 0, None]
    for i in (0, 1, 4, 5, 6, 7):
        assert h.gfv_lbfgs_pair(*[None if j == i else v for j, v in enumerate(good)]) == -1, i
    for i in (0, 1, 4, 5, 6, 7):
        assert h.gfv_lbfgs_pair(*[odd if j == i else v for j, v in enumerate(good)]) == -1, i
    assert h.gfv_lbfgs_pair(ok, ok, 130, n, ok, ok, ok, ok, 1.0, 0, None) == -1
    assert h.gfv_lbfgs_pair(ok, ok, slots, 1022, ok, ok, ok, ok, 1.0, 0, None) == -1
    assert h.gfv_lbfgs_pair(ok, ok, slots, 0, ok, ok, ok, ok, 1.0, 0, None) == -1
    # multidot(S, Y, slots, n, state, g, partial, mode, stream)
    good = [ok, ok, slots, n, ok, ok, ok, 0, None]
    for i in (0, 1, 4, 5, 6):
        assert h.gfv_lbfgs_multidot(*[None if j == i else v for j, v in enumerate(good)]) == -1, i
    for i in (0, 1, 4, 5, 6):
        assert h.gfv_lbfgs_multidot(*[odd if j == i else v for j, v in enumerate(good)]) == -1, i
    assert h.gfv_lbfgs_multidot(ok, ok, slots, n, ok, ok, ok, 3, None) == -1
    assert h.gfv_lbfgs_multidot(ok, ok, 1, n, ok, ok, ok, 0, None) == -1
    # coef(state, M, partial, delta, res, slots, n, mode, stream)
    good = [ok, ok, ok, ok, ok, slots, n, 0, None]
    for i in range(5):
        assert h.gfv_lbfgs_coef(*[None if j == i else v for j, v in enumerate(good)]) == -1, i
    for i in range(5):
        assert h.gfv_lbfgs_coef(*[odd if j == i else v for j, v in enumerate(good)]) == -1, i
    assert h.gfv_lbfgs_coef(ok, ok, ok, ok, ok, slots, n, -1, None) == -1
    # combine(S, Y, slots, n, state, g, delta, d, res, stream)
    good = [ok, ok, slots, n, ok, ok, ok, ok, ok, None]
    for i in (0, 1, 4, 5, 6, 7, 8):
        assert h.gfv_lbfgs_combine(*[None if j == i else v for j, v in enumerate(good)]) == -1, i
    for i in (0, 1, 4, 5, 6, 7, 8):
        assert h.gfv_lbfgs_combine(*[odd if j == i else v for j, v in enumerate(good)]) == -1, i
    # dot(a, mask, copy_out, b, n, partial, counter, out, stream)
    good = [ok, ok, ok, ok, n, ok, ok, ok, None]
    for i in (0, 1, 2, 3, 5, 6, 7):
        assert h.gfv_lbfgs_dot(*[None if j == i else v for j, v in enumerate(good)]) == -1, i
        assert h.gfv_lbfgs_dot(*[odd if j == i else v for j, v in enumerate(good)]) == -1, i
    assert h.gfv_lbfgs_dot(ok, ok, ok, ok, 1021, ok, ok, ok, None) == -1
    # axpy(p, x0, d, t, mask, n, stream)
    good = [ok, ok, ok, 1.0, ok, n, None]
    for i in (0, 1, 2, 4):
        assert h.gfv_lbfgs_axpy(*[None if j == i else v for j, v in enumerate(good)]) == -1, i
    for i in (0, 1, 2, 4):
        assert h.gfv_lbfgs_axpy(*[odd if j == i else v for j, v in enumerate(good)]) == -1, i
    assert h.gfv_lbfgs_axpy(ok, ok, ok, 1.0, ok + 1, n, None) == -1
    assert h.gfv_lbfgs_axpy(ok, ok, ok, 1.0, ok, -4, None) == -1
