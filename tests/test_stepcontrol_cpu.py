"""The adaptive time step (gfv/timescheme.py `StepControl`) without a GPU.

1. the constructor's checks, the 2.4 bound on `grow` for "bdf2" and its absence for "bdf1";
2. what the owners refuse;
3. the two entry points in the built library, in the binding and in include/gfv.h, the ABI version still 3;
4. the numpy rule (tests/stepcontrol_ref.py): the variable-step BDF2 difference is the exact derivative of a quadratic at the new
   level for unequal steps, its coefficients at omega = 1 are 1/3 and dt / 1.5, the controller's clamps, the rate of a uniform
   flow on one square cell, and a repeated clock."""
import os
import re
import types

import numpy as np
import pytest

import cases
import stepcontrol_ref as R

ERR_ARG = -1          # GFV_ERR_ARG of include/gfv.h
OMEGAS = (0.25, 0.5, 1.0, 1.5, 2.4)


# ---- 1. the constructor --------------------------------------------------------------------------------------------------------
def test_the_constructor_checks():
    from gfv.timescheme import BDF2_MAX_GROW, StepControl, TimeScheme
    c = StepControl()
    assert (c.courant, c.grow, c.shrink, c.min_factor, c.max_factor, c.keep) == (2.0, 1.5, 0.25, 0.05, 20.0, 1024)
    assert TimeScheme("bdf2").adapt is None and TimeScheme("bdf2", adapt=c).adapt is c
    StepControl(courant=0.1, grow=1, shrink=1, min_factor=1, max_factor=1, keep=1)
    for bad in (0, -1.0, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError, match="courant"):
            StepControl(courant=bad)
    for kw in (dict(shrink=0), dict(shrink=1.1), dict(grow=0.9), dict(shrink=-0.5), dict(grow=float("inf"))):
        with pytest.raises(ValueError, match="shrink|grow"):
            StepControl(**kw)
    for kw in (dict(min_factor=0), dict(min_factor=1.5), dict(max_factor=0.5), dict(max_factor=float("nan"))):
        with pytest.raises(ValueError, match="min_factor|max_factor"):
            StepControl(**kw)
    for bad in (0, -3, 1.5, True, None):
        with pytest.raises(ValueError, match="keep"):
            StepControl(keep=bad)
    # variable-step BDF2 is zero-stable for ratios below 1 + sqrt(2): the bound is on "bdf2" alone
    assert BDF2_MAX_GROW == 2.4 < 1 + np.sqrt(2)
    TimeScheme("bdf2", adapt=StepControl(grow=2.4))
    with pytest.raises(ValueError, match=r"zero-stable only for step ratios below 1 \+ sqrt\(2\)"):
        TimeScheme("bdf2", adapt=StepControl(grow=2.41))
    TimeScheme("bdf1", adapt=StepControl(grow=2.41))
    TimeScheme("bdf1", adapt=StepControl(grow=10.0))
    with pytest.raises(ValueError, match="StepControl or None"):
        TimeScheme("bdf2", adapt=2.0)
    sch = TimeScheme("bdf2", adapt=StepControl())
    for call in (sch.step_history, sch.read, sch.reset):
        with pytest.raises(RuntimeError, match="not attached"):
            call()


# ---- 2. the owners ---------------------------------------------------------------------------------------------------------------
def test_the_owners_refuse_followers_that_assume_a_constant_step():
    from gfv import timebc as T
    from gfv.fieldstats import FieldStats
    from gfv.march import MarchStep
    from gfv.pool_trainer import PoolTrainStep
    from gfv.timescheme import StepControl, TimeScheme, check_adapt_owner
    adaptive = lambda: TimeScheme("bdf2", adapt=StepControl())
    with pytest.raises(ValueError, match=r"adapt= together with time_bc=.*t = clock \* plan.dt"):
        MarchStep(None, None, time_scheme=adaptive(), time_bc=T.TimeBC(velocity=T.Ramp(0.5, 1.0, 0.0, 2.0, "smooth")))
    with pytest.raises(ValueError, match="adapt= together with field_stats=.*unweighted in time"):
        MarchStep(None, None, time_scheme=adaptive(), field_stats=FieldStats(start=1))
    # without adapt= neither is refused here (the constructor goes on to its next check and fails on the missing graphs)
    check_adapt_owner("MarchStep", TimeScheme("bdf2"), object(), object())
    check_adapt_owner("MarchStep", None, object(), object())
    check_adapt_owner("MarchStep", adaptive())
    with pytest.raises(ValueError, match="the pool owns the fields"):
        PoolTrainStep(None, None, time_scheme=adaptive())


# ---- 3. the entry points -----------------------------------------------------------------------------------------------------------
def test_the_library_declares_the_entry_points_and_the_abi_stays():
    from gfv import lib as L
    names = ("gfv_step_control_rate", "gfv_step_control_rows")
    assert set(names) <= set(L.declared_symbols())
    header = open(os.path.join(cases.ROOT, "include", "gfv.h")).read()
    for n in names:
        assert re.search(r"\bint " + n + r"\(", header), n
    assert int(re.search(r"#define GFV_ABI_VERSION (\d+)", header).group(1)) == 3 == L.ABI_VERSION
    for macro, v in (("RECORD", L.STEP_CONTROL_RECORD), ("PARAMS", L.STEP_CONTROL_PARAMS), ("STATE", L.STEP_CONTROL_STATE)):
        assert int(re.search(r"#define GFV_STEP_CONTROL_" + macro + r" (\d+)", header).group(1)) == v
    lib = L.load(raw=True)
    assert lib.gfv_abi_version() == 3
    # GFV_ERR_ARG before anything is launched: a NULL pointer, C / B / keep < 1, misaligned x_backup / kS / doubles
    a = 1 << 20
    good = [a] * 8 + [5, 2] + [a] * 14 + [4, None]
    ptrs = [i for i, v in enumerate(good) if v == a]
    assert len(ptrs) == 22
    for i in ptrs:
        args = list(good)
        args[i] = None
        assert lib.gfv_step_control_rate(*args) == ERR_ARG, i
    for i, v in ((8, 0), (9, 0), (24, 0), (0, a + 8), (5, a + 4), (15, a + 4), (18, a + 4), (23, a + 4)):
        args = list(good)
        args[i] = v
        assert lib.gfv_step_control_rate(*args) == ERR_ARG, i
    good = [a, a, a, 5, 2, a, a, a, a, a, None]
    for i in (0, 1, 2, 5, 6, 7, 8, 9):
        args = list(good)
        args[i] = None
        assert lib.gfv_step_control_rows(*args) == ERR_ARG, i
    for i, v in ((3, 0), (4, 0), (0, a + 8), (8, a + 4), (9, a + 4)):
        args = list(good)
        args[i] = v
        assert lib.gfv_step_control_rows(*args) == ERR_ARG, i


# ---- 4. the numpy rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("omega", OMEGAS)
def test_the_variable_step_difference_is_exact_on_a_quadratic(omega):
    """u(t) = a + b t + c t^2 sampled at t_{n-1} = t_n - dt_last, t_n, t_{n+1} = t_n + omega dt_last:
    (u_{n+1} - ustar) / dt_eff = u'(t_{n+1}) to float64 rounding."""
    g = np.random.default_rng(17)
    a, b, c = g.standard_normal((3, 50))
    t_n, dt_last = 0.7, 0.013
    dt_next = omega * dt_last
    u = lambda t: a + b * t + c * t * t
    u_prev, u_n, u_new = u(t_n - dt_last), u(t_n), u(t_n + dt_next)
    q, h = R.bdf2_divisors(np.float64(dt_next / dt_last))
    assert abs(1.0 / q - omega ** 2 / (1 + 2 * omega)) < 1e-15 and abs(1.0 / h - (1 + omega) / (1 + 2 * omega)) < 1e-15
    ustar, dt_eff = u_n + (u_n - u_prev) / q, dt_next / h
    exact = b + 2.0 * c * (t_n + dt_next)
    got = (u_new - ustar) / dt_eff
    # the difference of values of size |u| over a step dt_eff: rounding of the samples is amplified by |u| / dt_eff
    bound = 64 * np.finfo(np.float64).eps * float(np.abs(u_new).max()) / dt_eff
    err = float(np.abs(got - exact).max())
    print(f"omega {omega}: max error {err:.2e}, bound {bound:.2e}, max |u'| {float(np.abs(exact).max()):.2f}")
    assert err <= bound
    # the first-order form on the same samples misses it by c dt: the test can tell the two apart
    assert float(np.abs((u_new - u_n) / dt_next - exact).max()) > 1e6 * bound


def test_at_unit_ratio_the_coefficients_are_exactly_one_third_and_dt_over_one_and_a_half():
    for dtype in (np.float64, np.float32):
        q, h = R.bdf2_divisors(dtype(1.0), dtype)
        assert q.dtype == dtype and q == 3.0 and h == 1.5
        d, dt = dtype(0.37), dtype(0.0125)
        assert d / q == d / dtype(3.0) and dt / h == dt / dtype(1.5)
    assert 1.0 / R.bdf2_divisors(1.0)[0] == 1.0 / 3.0


def test_the_controller_and_each_of_its_clamps():
    ctl = types.SimpleNamespace(courant=2.0, grow=1.5, shrink=0.25, min_factor=0.5, max_factor=4.0)
    dt_plan = np.full(6, 0.01)
    #                 in band   grow   shrink   zero -> grow   max_factor   min_factor
    rate = np.array([160.0,    10.0,  4000.0,  0.0,           10.0,        4000.0])
    last = np.array([0.01,     0.01,  0.01,    0.01,          0.035,       0.012])
    co, dt_next, omega = R.controller(rate, last, dt_plan, ctl)
    np.testing.assert_allclose(co, rate * last, rtol=0, atol=0)
    np.testing.assert_allclose(dt_next, [0.0125, 0.015, 0.0025 * 2, 0.015, 0.04, 0.005], rtol=1e-15)
    np.testing.assert_allclose(omega, dt_next / last, rtol=0, atol=0)
    # (column 2: shrink gives 0.0025, below min_factor * dt = 0.005 - both clamps; column 5: shrink gives 0.003)
    assert omega[0] == 1.25 and omega[1] == 1.5 == omega[3] and omega[4] < 1.5 and omega[5] > 0.25
    # the target is reached in one step when no clamp is hit
    assert abs(rate[0] * dt_next[0] - ctl.courant) < 1e-12


def _one_square():
    """One unit-square cell of four nodes with outward face vectors, twice: graph 0 moves, graph 1 is at rest."""
    kS1 = np.array([[0.0, -1.0], [1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]])
    plan = {"batch": np.repeat([0, 1], 4), "uvp_dim": np.array([[2.0, 4.0, 1.0], [1.0, 1.0, 1.0]]), "dt": np.array([0.01, 0.02]),
            "crow": np.array([0, 4, 8]), "knode": np.arange(8), "kS": np.concatenate((kS1, kS1)), "area": np.array([1.0, 1.0]),
            "cbatch": np.array([0, 1])}
    x = np.zeros((8, 12))
    x[0:4, 0], x[0:4, 1] = 3.0, -2.0          # dimensionless (1.5, -0.5) everywhere in graph 0
    return plan, x


def test_the_rate_of_a_uniform_flow_and_a_repeated_clock():
    plan, x = _one_square()
    rates = R.cell_rates(x, plan["uvp_dim"], plan["crow"], plan["knode"], plan["kS"], plan["area"], plan["cbatch"])
    # sum_k |u . S_k| / (2 A) = (2 |u| + 2 |v|) / 2 = |u| / dx + |v| / dy on a unit square
    assert rates.tolist() == [2.0, 0.0]
    ctl = types.SimpleNamespace(courant=0.5, grow=2.0, shrink=0.25, min_factor=0.05, max_factor=20.0)
    rule = R.StepRule(plan, ctl, R.BDF2)
    rule.reset(0)
    first = rule.launch(x, 0)
    assert not first["active"] and first["time"].tolist() == [0.0, 0.0]
    assert first["courant"].tolist() == [0.02, 0.0]                       # at the base the step behind the field is the plan's
    assert first["dt"].tolist() == [0.02, 0.04] and first["omega"].tolist() == [2.0, 2.0]      # grow, and Co = 0: grow
    again = rule.launch(x, 0)
    for k in first:
        assert np.array_equal(np.asarray(first[k]), np.asarray(again[k])), k
    x1 = x.copy()
    x1[:, 0:2] *= 0.5
    second = rule.launch(x1, 1)
    assert second["active"] and second["dt_last"].tolist() == [0.02, 0.04] and second["time"].tolist() == [0.02, 0.04]
    assert second["courant"].tolist() == [0.02, 0.0] and second["omega"].tolist() == [2.0, 2.0]
    q, h = R.bdf2_divisors(2.0)
    assert (q, h) == (1.25, 5.0 / 3.0)                                    # the weights 0.8 and 0.6
    np.testing.assert_allclose(second["ustar"][0], [0.75 + 0.8 * (0.75 - 1.5), -0.25 + 0.8 * (-0.25 + 0.5)], rtol=1e-15)
    np.testing.assert_allclose(second["dt_eff"], [0.04 * 0.6, 0.08 * 0.6], rtol=1e-15)
    again = rule.launch(x1, 1)
    for k in second:
        assert np.array_equal(np.asarray(second[k]), np.asarray(again[k])), k
    assert [rule.history[c]["time"].tolist() for c in (0, 1)] == [[0.0, 0.0], [0.02, 0.04]]
