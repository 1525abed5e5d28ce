"""GPU: `gfv.optstep.optimizer_launches` against the C entries of its table called directly, in the table's order,
on a bit-identical second set of buffers - all 16 combinations of accumulation (A), active guard (G), averaged weights (E) and
parameter groups (P), three steps each, every buffer and every device record compared bit for bit.

Two sizes, the smallest at which the grids can differ: n = 5 is one workgroup (which is also the last to arrive) and, in the
accumulate kernel, one float4 plus the scalar tail; n = 512 * 512 + 517 reaches the Adam grid's cap of 512 workgroups of 512
threads, so the grid-stride loop wraps.  accum_steps = 2 gives a hold, a closing and again a hold micro-step; max_grad_norm = 0.5
is below the norm of every gradient here (about sqrt(n) >= 2), so the guard clips - asserted from its record."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = {5: [0, 2, 4], 512 * 512 + 517: [0, 131, 512 * 512 + 5]}   # n: where the three runs start
RUN_GROUP = [0, 1, 0]                                              # three runs in two groups
GROUP_VALUES = [(1e-3, 0.0, False), (3e-3, 0.1, False)]            # (lr, weight_decay, frozen): the second group decays
BETAS, EPS, STEPS, B = (0.9, 0.999), 1e-8, 3, 3


class _Layout:
    """What GradGuard and ParamGroups read of a gfv.engine.GradStore: three 1-D tensors back to back (no alignment padding, so
    that n is exactly the size under test)."""

    def __init__(self, n):
        starts = SIZES[n]
        self.total, self.skip = n, set()
        self.off = {str(i): s for i, s in enumerate(starts)}
        self.shape = {str(i): (e - s,) for i, (s, e) in enumerate(zip(starts, starts[1:] + [n]))}

    def numel(self, name):
        return self.shape[name][0]


_INPUTS = {}


def _inputs(n):
    """(start parameters, [gradient per step], [loss per step]) on the host; computed once per size."""
    if n not in _INPUTS:
        gen = torch.Generator().manual_seed(1000 + n % 997)
        _INPUTS[n] = (torch.randn(n, generator=gen), [torch.randn(n, generator=gen) * (1 + s) for s in range(STEPS)],
                      [torch.rand(1, generator=gen) for _ in range(STEPS)])
    return _INPUTS[n]


class _Side:
    def __init__(self, n, A, G, E, P):
        from gfv import lib as L
        from gfv.accum import GradAccum
        from gfv.ema import WeightEMA
        from gfv.groups import ParamGroups
        from gfv.guard import GradGuard
        layout = _Layout(n)
        self.n = n
        self.p = _inputs(n)[0].cuda()
        self.m, self.v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        self.g = torch.zeros(n, device="cuda")
        self.loss = torch.zeros(1, device="cuda")
        self.state = torch.zeros(16, device="cuda")
        L.check(L.load().gfv_adam_state_init(self.state.data_ptr(), *BETAS, 0.0, L.stream_ptr()), "adam_state_init")
        self.hyper = torch.tensor([1e-3, *BETAS, EPS, 1.0, 0.0, 0.0, 0.0], device="cuda")
        self.guard = GradGuard(layout, "cuda", max_grad_norm=0.5 if G else None)
        self.accum = GradAccum(n, "cuda", 2) if A else None
        self.ema = WeightEMA(self.p, n, 0.9, True) if E else None
        self.groups = ParamGroups(layout, "cuda", {str(i): r for i, r in enumerate(RUN_GROUP)}, GROUP_VALUES, True) if P else None
        assert self.guard.active == G and (self.guard.n_seg, self.guard.n_elems) == (1, n)

    def feed(self, step):
        _, grads, losses = _inputs(self.n)
        self.g.copy_(grads[step])
        self.loss.copy_(losses[step])

    def bits(self):
        torch.cuda.synchronize()
        out = {"p": self.p, "m": self.m, "v": self.v, "g": self.g, "adam_state": self.state, "guard": self.guard.guard}
        if self.accum is not None:
            out.update(acc=self.accum.acc, accum=self.accum.rec)
        if self.ema is not None:
            out.update(e=self.ema.e, ema=self.ema.rec)
        return {k: t.detach().cpu().view(torch.int32).clone() for k, t in out.items()}


def _table_entries(s, A, G, E, P):
    """The table of DESIGN.md 5f through the C ABI itself."""
    from gfv import lib as L
    lib, st = L.load(), L.stream_ptr()
    p, g, m, v, state, hyper = (t.data_ptr() for t in (s.p, s.g, s.m, s.v, s.state, s.hyper))
    arec = s.accum.rec.data_ptr() if A else None
    grec = s.guard.guard.data_ptr() if G else None
    e, erec = (s.ema.e.data_ptr(), s.ema.rec.data_ptr()) if E else (None, None)
    if A:
        L.check(lib.gfv_grad_accum_dev(g, s.accum.acc.data_ptr(), s.n, B, s.loss.data_ptr(), arec, st), "grad_accum")
    if G:
        norm = (g, s.guard.segs.data_ptr(), s.guard.n_seg, s.guard.n_elems, hyper, grec, s.guard.ws.data_ptr())
        if A:
            L.check(lib.gfv_grad_guard_accum_dev(*norm, arec, st), "grad_guard_accum")
        else:
            L.check(lib.gfv_grad_guard_dev(*norm, st), "grad_guard")
    if P:
        L.check(lib.gfv_adam_step_groups_dev(p, g, m, v, e, s.n, state, hyper, grec, arec, erec, s.groups.run_start.data_ptr(),
                                             s.groups.run_group.data_ptr(), s.groups.n_runs, s.groups.table.data_ptr(), st),
                "adam_step_groups")
    elif E:
        L.check(lib.gfv_adam_step_ema_dev(p, g, m, v, e, s.n, state, hyper, grec, arec, erec, st), "adam_step_ema")
    elif A:
        L.check(lib.gfv_adam_step_accum_dev(p, g, m, v, s.n, state, hyper, grec, arec, st), "adam_step_accum")
    elif G:
        L.check(lib.gfv_adam_step_guarded_dev(p, g, m, v, s.n, state, hyper, grec, st), "adam_step_guarded")
    else:
        L.check(lib.gfv_adam_step_dev(p, g, m, v, s.n, state, hyper, st), "adam_step")


@pytest.mark.parametrize("A,G,E,P", list(itertools.product((False, True), repeat=4)))
@pytest.mark.parametrize("n", list(SIZES))
def test_optimizer_launches_is_the_table_bit_for_bit(n, A, G, E, P):
    from gfv.optstep import optimizer_launches
    a, b = _Side(n, A, G, E, P), _Side(n, A, G, E, P)
    start = a.bits()
    assert all(torch.equal(start[k], t) for k, t in b.bits().items())
    for step in range(STEPS):
        a.feed(step)
        b.feed(step)
        optimizer_launches(a.p, a.g, a.m, a.v, n, a.state, a.hyper, guard=a.guard, accum=a.accum, ema=a.ema, groups=a.groups,
                           B=B, loss=a.loss)
        _table_entries(b, A, G, E, P)
    got, want = a.bits(), b.bits()
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    # the run did what it was set up to do: one closed accumulation of two (a hold step on either side of it), or three steps;
    # a clip at every decision; the average advanced with every applied step; the parameters moved
    applied = 1 if A else STEPS
    assert float(a.state[0]) == applied
    assert not torch.equal(got["p"], start["p"])
    if A:
        assert int(got["accum"][6]) == 1 and int(got["accum"][1]) == 1
    if G:
        assert int(got["guard"][5]) == applied and int(got["guard"][6]) == 0
    if E:
        assert int(got["ema"][2]) == applied
