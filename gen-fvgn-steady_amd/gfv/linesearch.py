"""Strong-Wolfe line search on host scalars (Nocedal & Wright, Numerical Optimization, algorithms 3.5 / 3.6), with the cubic
interpolation, the bracket rules and the safeguards of torch.optim.LBFGS's search, so that the same scalar problem gives the
same step and the same number of evaluations.

The search knows nothing about vectors: `phi(t) -> (f, gtd)` evaluates the objective and its directional derivative at step
`t`.  A caller that keeps per-point data (gfv.optim.LBFGS keeps the gradient of every live point in a device slot) passes
`keep`: it is called before every evaluation with the steps whose data the search may still return - the caller may recycle
everything else.  The returned step is always one of the evaluated points or 0.
"""
from __future__ import annotations

import math


def cubic_interpolate(x1, f1, g1, x2, f2, g2, bounds=None):
    """Minimiser of the cubic through (x1, f1, g1) and (x2, f2, g2), clamped to `bounds` (default: between the points); the
    middle of the bounds where the cubic has no minimum."""
    if bounds is not None:
        lo, hi = bounds
    else:
        lo, hi = (x1, x2) if x1 <= x2 else (x2, x1)
    d1 = g1 + g2 - 3 * (f1 - f2) / (x1 - x2)
    d2_square = d1 ** 2 - g1 * g2
    if d2_square >= 0:
        d2 = math.sqrt(d2_square)
        if x1 <= x2:
            min_pos = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2))
        else:
            min_pos = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2 * d2))
        return min(max(min_pos, lo), hi)
    return (lo + hi) / 2.0


def strong_wolfe(phi, t, f0, gtd0, c1=1e-4, c2=0.9, tolerance_change=1e-9, max_ls=25, d_norm=1.0, keep=None):
    """Returns (f, t, evaluations).  `f0`, `gtd0`: objective and directional derivative at t = 0; `d_norm`: max|d| of the
    direction (the bracket is given up once |bracket| * d_norm < tolerance_change; 1 for a scalar problem)."""
    t = float(t)
    f0, gtd0 = float(f0), float(gtd0)
    if keep is not None:
        keep((0.0,))
    f_new, gtd_new = phi(t)
    evals = 1

    # bracketing phase (alg. 3.5): grow t until an interval holds a point that satisfies the conditions
    t_prev, f_prev, gtd_prev = 0.0, f0, gtd0
    done = False
    ls_iter = 0
    bracket = bracket_f = bracket_gtd = None
    while ls_iter < max_ls:
        if f_new > (f0 + c1 * t * gtd0) or (ls_iter > 1 and f_new >= f_prev):
            bracket, bracket_f, bracket_gtd = [t_prev, t], [f_prev, f_new], [gtd_prev, gtd_new]
            break
        if abs(gtd_new) <= -c2 * gtd0:
            bracket, bracket_f = [t], [f_new]
            done = True
            break
        if gtd_new >= 0:
            bracket, bracket_f, bracket_gtd = [t_prev, t], [f_prev, f_new], [gtd_prev, gtd_new]
            break
        min_step = t + 0.01 * (t - t_prev)
        max_step = t * 10
        tmp = t
        t = cubic_interpolate(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, bounds=(min_step, max_step))
        t_prev, f_prev, gtd_prev = tmp, f_new, gtd_new
        if keep is not None:
            keep((0.0, t_prev))     # (t = 0 stays: it is one end of the bracket if the evaluations run out)
        f_new, gtd_new = phi(t)
        evals += 1
        ls_iter += 1

    if ls_iter == max_ls:
        bracket, bracket_f = [0.0, t], [f0, f_new]

    # zoom phase (alg. 3.6): shrink the bracket until a point satisfies the conditions
    insuf_progress = False
    low_pos, high_pos = (0, 1) if bracket_f[0] <= bracket_f[-1] else (1, 0)
    while not done and ls_iter < max_ls:
        if abs(bracket[1] - bracket[0]) * d_norm < tolerance_change:
            break
        t = cubic_interpolate(bracket[0], bracket_f[0], bracket_gtd[0], bracket[1], bracket_f[1], bracket_gtd[1])
        # a trial point within a tenth of the bracket of one of its ends: accepted once, moved inwards the second time or when
        # it sits on the end itself
        hi, lo = max(bracket), min(bracket)
        eps = 0.1 * (hi - lo)
        if min(hi - t, t - lo) < eps:
            if insuf_progress or t >= hi or t <= lo:
                t = hi - eps if abs(t - hi) < abs(t - lo) else lo + eps
                insuf_progress = False
            else:
                insuf_progress = True
        else:
            insuf_progress = False

        if keep is not None:
            keep(tuple(bracket))
        f_new, gtd_new = phi(t)
        evals += 1
        ls_iter += 1

        if f_new > (f0 + c1 * t * gtd0) or f_new >= bracket_f[low_pos]:
            bracket[high_pos], bracket_f[high_pos], bracket_gtd[high_pos] = t, f_new, gtd_new
            low_pos, high_pos = (0, 1) if bracket_f[0] <= bracket_f[1] else (1, 0)
        else:
            if abs(gtd_new) <= -c2 * gtd0:
                done = True
            elif gtd_new * (bracket[high_pos] - bracket[low_pos]) >= 0:
                bracket[high_pos], bracket_f[high_pos], bracket_gtd[high_pos] = \
                    bracket[low_pos], bracket_f[low_pos], bracket_gtd[low_pos]
            bracket[low_pos], bracket_f[low_pos], bracket_gtd[low_pos] = t, f_new, gtd_new

    return bracket_f[low_pos], bracket[low_pos], evals
