"""The launches of one optimiser step, in the one place that knows their order (include/gfv.h gfv_adam_step_dev).
`gfv.trainer.TrainStep._adam()` and `gfv.optim.Adam.step()` end here; the record owners - `gfv.guard.GradGuard`,
`gfv.accum.GradAccum`, `gfv.ema.WeightEMA`, `gfv.groups.ParamGroups` - hold device records and tables and issue nothing.

With A = accumulation on, G = guard active, E = averaged weights on, P = parameter groups on:

  1. A:  gfv_grad_accum_dev
  2. G:  gfv_grad_guard_accum_dev if A else gfv_grad_guard_dev
  3. the Adam entry - guard given iff G, accum iff A, e and ema iff E:
       P               gfv_adam_step_groups_dev
       E               gfv_adam_step_ema_dev
       A               gfv_adam_step_accum_dev
       G               gfv_adam_step_guarded_dev
       none of them    gfv_adam_step_dev

The entry per form is fixed: it decides the kernel instantiation, and with it the bits of the step.

H = `hold` given (gfv/march.py): a device record whose word [3] is an apply flag that SOMEBODY ELSE's launch has
written in front of these.  It goes where accum's record goes in 2 and 3 - the guard's `_accum` entry, the Adam entry as with A -
and launch 1 is not issued: of that record the launches of 2 and 3 read word [3] alone (csrc/misc.hip AC_APPLY; include/gfv.h).
With the flag at 1 their results are those of the forms without a record, bit for bit."""
from __future__ import annotations

from . import lib as L


def optimizer_launches(p, g, m, v, n, state, hyper, *, guard=None, accum=None, ema=None, groups=None, B=1, loss=None, hold=None):
    """p, g, m, v: flat fp32 tensors of n elements; state, hyper: the Adam step record and the hyper-parameters; guard, accum,
    ema, groups: the record owners or None (a guard counts only when `.active`); B, loss: graph count and device loss of this
    micro-batch, read by the accumulate launch only; hold: a device tensor of at least 4 32-bit words, word [3] the apply flag
    (not together with accum: the two would claim the same argument)."""
    if hold is not None and accum is not None:
        raise ValueError("optimizer_launches: hold= and accum= both name the record the Adam launch reads its apply flag from")
    lib, st = L.load(), L.stream_ptr()
    gp, hp = g.data_ptr(), hyper.data_ptr()
    arec = None
    if accum is not None:
        arec = accum.rec.data_ptr()
        L.check(lib.gfv_grad_accum_dev(gp, accum.acc.data_ptr(), n, int(B), loss.data_ptr(), arec, st), "grad_accum")
    elif hold is not None:
        arec = hold.data_ptr()
    grec = None
    if guard is not None and guard.active:
        grec = guard.guard.data_ptr()
        norm = (gp, guard.segs.data_ptr(), guard.n_seg, guard.n_elems, hp, grec, guard.ws.data_ptr())
        if arec is None:
            L.check(lib.gfv_grad_guard_dev(*norm, st), "grad_guard")
        else:
            L.check(lib.gfv_grad_guard_accum_dev(*norm, arec, st), "grad_guard_accum")
    e, erec = (None, None) if ema is None else (ema.e.data_ptr(), ema.rec.data_ptr())
    pmv = (p.data_ptr(), gp, m.data_ptr(), v.data_ptr())
    sp = state.data_ptr()
    if groups is not None:
        L.check(lib.gfv_adam_step_groups_dev(*pmv, e, n, sp, hp, grec, arec, erec, groups.run_start.data_ptr(),
                                             groups.run_group.data_ptr(), groups.n_runs, groups.table.data_ptr(), st),
                "adam_step_groups")
    elif ema is not None:
        L.check(lib.gfv_adam_step_ema_dev(*pmv, e, n, sp, hp, grec, arec, erec, st), "adam_step_ema")
    elif arec is not None:
        L.check(lib.gfv_adam_step_accum_dev(*pmv, n, sp, hp, grec, arec, st), "adam_step_accum")
    elif grec is not None:
        L.check(lib.gfv_adam_step_guarded_dev(*pmv, n, sp, hp, grec, st), "adam_step_guarded")
    else:
        L.check(lib.gfv_adam_step_dev(*pmv, n, sp, hp, st), "adam_step")
