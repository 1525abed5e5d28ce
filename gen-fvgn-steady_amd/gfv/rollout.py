"""Forward-only rollout: advance a trained model in time, saving nothing.

The reference runs a trained model with `solve_without_grad_GPU.py:117-173`: call the model, keep the predicted field, write
`graph_node.x = cat(uvp_node_new.detach(), backup[:, 3:])`, call it again - and never calls `backward()`.  `Rollout` is that
loop on the forward-only engine path (`Engine.forward(keep=False)`: the launches of the training forward on the same kernel
families, with NULL for every tensor only a backward would read - bit-identical outputs) with one launch behind it
(`gfv_rollout_advance`, csrc/rollout.hip) that does the write-back, restores the un-normalised node state and appends the
step's residual losses and update norms to a device-resident history.

    r = Rollout(model, graphs, max_steps=1000)
    losses, uvp_node, uvp_cell = r.step()
    hist = r.run(steps=200, tol=1e-6, check_every=50)      # [k, B, 6]: four losses, ||d uvp||_2, ||uvp||_2 per graph

Launch modes.  "cmd_list" (default): the step is issued eagerly twice (which settles the weight-image set), recorded once with
`gfv.cmdlist.record` and replayed from then on; "eager": launch by launch.  The two give the same bits.

Who owns what a recorded list points at: DESIGN.md 5l.  Particular to this object, created in set-up and held for its lifetime,
never reallocated: `x`, `x_backup`, the history, the step counter, the reduction workspace, the plan and the graphs.

Weights.  Images (and, for hidden_size < 128, the padded copies) are built ONCE - in the constructor and in
`refresh_weights()` - not per step (gfv/static_forward.py).  Each `step()` raises on a parameter or engine change instead of
replaying stale images: after `load_state_dict`, an optimizer step or `.to()`, call `refresh_weights()`.

Normalizer.  As in the reference loop the model is called with `norm_global` every step, and `accumulate` follows
`node_norm.should_accumulate()` exactly as `NNmodel.forward` does - for a trained model (accumulation count reached) that is
"never".  A recorded list is made for ONE of the two values; when it flips (the count is reached during a rollout) the other
list is warmed up and recorded.

Anderson acceleration (`anderson=m`, 1 .. 8; gfv/anderson.py).  For the STEADY iteration: the rollout is the
fixed-point iteration x_{k+1} = G(x_k), and with `anderson=m` two more launches between the forward and the advance mix the
model's output with the last m residual differences per graph, decided on the device (nothing in them depends on the host: one
recorded list serves every step).  `step()` then returns the iterate the rollout advanced to (uvp_node is overwritten in place;
the losses and uvp_cell are the model's for the state it was given), history columns 4 / 5 hold the ACCELERATED update, and
`run(tol=...)` tests the true fixed-point residual || G(x) - x || / || G(x) || of `anderson_history()` instead.  The accelerated
iterates are not time steps of the model: a time-accurate unsteady rollout must leave it off.  The defaults
`anderson_reg=1e-10` and `anderson_restart=10` are those of a CPU experiment on linear contractions; they have not been tuned on
a trained model.  `anderson=0` (the default) issues no new launch and allocates nothing.

Field statistics (`field_stats=FieldStats(start=, stride=, stop=)`; gfv/fieldstats.py).  For the UNSTEADY rollout: one
more launch behind the advance samples the field just written into per-node running sums - time mean, variances, u'v', extremes -
following the step counter (the field step k leaves has clock k, the first is 1).  Eager steps and recorded lists carry it alike;
`r.field_stats.read()` is the one synchronisation, `set_window()` moves the window under a recorded list.  Refused together with
`anderson` > 0.  `field_stats=None` (the default) issues no new launch and allocates nothing.

Unsteady boundary data (`time_bc=TimeBC(velocity=, source=, nodes=)`; gfv/timebc.py).  One more launch behind the
advance rewrites the Dirichlet velocity targets and the source coefficient for the step about to be taken, from per-graph waveform
records on the device (a ramped start-up, a pulsatile inlet, an oscillating lid, a pulsating body force), following the step
counter.  Eager steps and recorded lists carry it alike; `r.time_bc.read()` is what was applied, `set()` changes a waveform under
a recorded list.  Refused together with `anderson` > 0 and for graphs of a DevicePool.  `time_bc=None` (the default) issues no
new launch and allocates nothing.

Wall forces (`wall_forces=WallForces(faces=, box=, origin=, start=, stride=, stop=, keep=)`; gfv/wallforce.py).  Two more
launches behind the advance, beside the field-statistics launch and before the boundary-data launch, sum the pressure and the viscous
force of the field just written over the selected wall faces, and their moments, per graph, into a device ring of the last `keep`
samples - the drag and lift history of a cylinder or airfoil run - following the step counter.  Eager steps and recorded lists carry
them alike; `r.wall_forces.read()` is the one synchronisation, `set_window()` moves the window under a recorded list.  Refused together
with `anderson` > 0 (a steady user calls `gfv.wallforce.evaluate()` on the converged field) and for graphs of a DevicePool; allowed
beside `field_stats` and `time_bc`.  `wall_forces=None` (the default) issues no new launch and allocates nothing.

Probes (`probes=Probes(points, graph=, start=, stride=, stop=, keep=, tolerance=)`; gfv/probes.py).  One more launch
behind the advance, after the wall-force pair and before the boundary-data launch, interpolates (u, v, p) and their gradients of the
field just written at fixed points of the mesh - located, and their weights built, once when the object is attached - into a device
ring of the last `keep` samples, following the step counter.  Eager steps and recorded lists carry it alike; `r.probes.read()` is the
one synchronisation, `set_window()` moves the window under a recorded list.  Refused together with `anderson` > 0 (a steady user calls
`gfv.probes.sample()` on the converged field) and for graphs of a DevicePool; allowed beside every other follower.  `probes=None`
(the default) issues no new launch and allocates nothing.

Flow integrals (`integrals=FlowIntegrals(start=, stride=, stop=, keep=, fields=)`; gfv/integrals.py).  One more launch
behind the advance, after the wall-force pair and before the probes, sums per graph the kinetic energy, the enstrophy, the norms of
the discrete divergence, the circulation, the pressure integral and the flux through the inflow, outflow and other boundary faces of
the field just written into a device ring of the last `keep` samples, following the step counter; with `fields=True` it also keeps
the cell vorticity and divergence of the latest sample.  Eager steps and recorded lists carry it alike; `r.integrals.read()` is the
one synchronisation, `set_window()` moves the window under a recorded list.  Refused together with `anderson` > 0 (a steady user calls
`gfv.integrals.evaluate()` on the converged field) and for graphs of a DevicePool; allowed beside every other follower.
`integrals=None` (the default) issues no new launch and allocates nothing.
"""
from __future__ import annotations

import torch

from . import anderson as AA
from . import cmdlist
from . import lib as L
from .fieldstats import FieldStats
from .follow import check_followers
from .functions import require_gpu
from .listcache import WARM, ListCache
from .plan import get_plan
from .static_forward import StaticForward, WeightGuard  # noqa: F401  (WeightGuard: named from here by its users)

HISTORY_WIDTH = 6   # (loss_cont, loss_mom_x, loss_mom_y, loss_press, ||uvp_new - uvp_prev||_2, ||uvp_new||_2) per graph


def check_room(steps_done, max_steps, steps=1):
    """The history holds `max_steps` rows: a step that would write past it is refused on the host (the kernel would skip the
    row, but the caller asked for a record of every step)."""
    if steps_done + steps > max_steps:
        raise IndexError(f"Rollout: {steps_done} steps done + {steps} asked for exceeds max_steps={max_steps} "
                         "(the device history has one row per step); reset() or build the Rollout with a larger max_steps")


def check_field_stats(field_stats, anderson):
    """What a Rollout refuses of `field_stats=`; needs no GPU."""
    FieldStats.check_handed("Rollout", field_stats, None, anderson)


class Rollout:
    WARM = WARM   # eager steps before a list is recorded (they are steps of the rollout like any other)

    def __init__(self, model, graphs, max_steps=1000, launch_mode="cmd_list", norm_global=None, anderson=0, anderson_beta=1.0,
                 anderson_reg=1e-10, anderson_restart=10.0, anderson_start=0, field_stats=None, time_bc=None,
                 wall_forces=None, probes=None, integrals=None):
        if launch_mode not in ("cmd_list", "eager"):
            raise ValueError('launch_mode must be "cmd_list" or "eager"')
        aa_args = AA.check_args(anderson, anderson_beta, anderson_reg, anderson_restart, anderson_start)
        check_followers("Rollout", graphs, aa_args[0], field_stats=field_stats, wall_forces=wall_forces, time_bc=time_bc,
                        integrals=integrals, probes=probes)
        graph_node = graphs[0]
        x = graph_node.x
        require_gpu(x)
        if int(max_steps) < 1:
            raise ValueError("max_steps must be at least 1")
        if not getattr(graph_node, "norm_uvp", True):
            raise ValueError("Rollout needs the un-normalised node state (graph.norm_uvp is False: the features have already "
                             "been normalised by a forward)")
        self.model, self.graphs = model, graphs
        self.launch_mode = launch_mode
        self.max_steps = int(max_steps)
        self.engine = model.engine()
        self.plan = get_plan(graphs)
        dev = x.device
        self.dev = dev
        pl = self.plan
        if norm_global is None:
            norm_global = bool(getattr(graph_node, "norm_global", getattr(model.params, "norm_global", True)))
        self.norm_global = bool(norm_global)
        # state: the un-normalised rows (x_backup: what the input preparation reads) and the tensor it normalises into
        self.x_backup = x.detach().to(torch.float32).contiguous().clone()
        self._x0 = self.x_backup.clone()
        self.x = self.x_backup.clone()
        self.history = torch.zeros((self.max_steps, pl.B, HISTORY_WIDTH), dtype=torch.float32, device=dev)
        self._state = torch.zeros(2, dtype=torch.int32, device=dev)          # (step counter, arrival counter)
        self._partial = torch.zeros((pl.n_chunks, 2), dtype=torch.float64, device=dev)
        L.status_mirror()
        self.anderson = aa_args[0]
        self._aa = AA.AndersonState(pl, dev, self.max_steps, *aa_args) if self.anderson else None
        self.steps_done = 0
        self._lists = ListCache(None, dev=dev)      # accumulate -> the recorded step; unbounded: two keys at most
        self._outs = None
        self._fwd = StaticForward(model, pl.B, dev)
        # The followers of the step counter (gfv/follow.py; word 0 of _state), attached last: should a line above raise, they stay
        # free for another owner.  Behind the advance field_stats samples the field just written, wall_forces, integrals and probes read it and the
        # plan and write only their own state, time_bc writes the targets of step counter + 1 (its attach: those of step 1, the counter is 0).
        self.field_stats = field_stats and field_stats.attach(self, self.x_backup, self._state, 0)
        self.wall_forces = wall_forces and wall_forces.attach(self, graphs, pl, self.x_backup, self._state, 0)
        self.integrals = integrals and integrals.attach(self, graphs, pl, self.x_backup, self._state, 0)
        self.probes = probes and probes.attach(self, graphs, pl, self.x_backup, self._state, 0)
        self.time_bc = time_bc and time_bc.attach(self, graphs, pl, self.x_backup, self.x, self._state, 0, self.max_steps)
        self._followers = [f for f in (self.field_stats, self.wall_forces, self.integrals, self.probes, self.time_bc)
                           if f is not None]

    # ---- weights -------------------------------------------------------------------------------------------------------
    def refresh_weights(self):
        """(Re)build what depends on the parameter VALUES: padded copies (hidden_size < 128) and the forward weight images.
        Recorded lists are dropped (the next steps warm up and record again)."""
        self._fwd.refresh()
        self._lists.clear()

    P = property(lambda self: self._fwd.P)

    # ---- one step ------------------------------------------------------------------------------------------------------
    def _body(self, acc):
        pl = self.plan
        losses, uvp_node, uvp_cell = self._fwd.forward(self.x, self.x_backup, pl, acc, self.norm_global)
        if self._aa is not None:
            self._aa.launch(uvp_node, self.x_backup, self._state)
        L.check(L.load().gfv_rollout_advance(
            uvp_node.data_ptr(), self.x_backup.data_ptr(), self.x.data_ptr(), pl.N, pl.chunk_beg.data_ptr(),
            pl.chunk_end.data_ptr(), pl.gchunk_ptr.data_ptr(), pl.n_chunks, pl.B, losses.data_ptr(), self._partial.data_ptr(),
            self.history.data_ptr(), self.max_steps, self._state.data_ptr(), L.stream_ptr()), "gfv_rollout_advance")
        for f in self._followers:
            f.launch()
        L.status_publish()
        return losses, uvp_node, uvp_cell

    def step(self):
        """One forward-only step + advance -> (losses [B,4], uvp_node [N,3], uvp_cell [C,3]).  In list mode the three are the
        recorded step's own tensors: the next step overwrites them.  With `anderson` > 0 uvp_node is the iterate the rollout
        advanced to (the mixed one where the step was accelerated)."""
        L.raise_on_status("Rollout.step")
        check_room(self.steps_done, self.max_steps)
        self._fwd.check("Rollout", "rollout")
        norm = self.model.node_norm
        acc = self.norm_global and norm.should_accumulate()
        # (a recording or a stream capture that is already open takes the step eagerly, and counts no warm-up)
        listed = self.launch_mode == "cmd_list" and cmdlist.active() is None and not torch.cuda.is_current_stream_capturing()
        outs = self._lists.run(acc, lambda: self._body(acc), listed)
        if acc:
            norm.note_accumulated()
        self.steps_done += 1
        self._outs = outs
        return outs

    def run(self, steps, tol=None, check_every=50):
        """`steps` steps -> the history so far as a CPU tensor [k, B, 6].  tol: stop early once every graph's relative update
        ||d uvp||_2 / ||uvp||_2 of the latest step is below it at a check - every `check_every` steps and after the last one;
        a check is the only synchronisation (none at all without tol, until the history is copied out).  With `anderson` > 0
        the test is on the true fixed-point residual || G(x) - x ||_2 / || G(x) ||_2 of the latest step (`anderson_history()`
        columns 0 / 1): history columns 4 / 5 then hold the accelerated update."""
        steps = int(steps)
        check_room(self.steps_done, self.max_steps, steps)
        check_every = max(1, int(check_every))
        for i in range(steps):
            self.step()
            if tol is not None and ((i + 1) % check_every == 0 or i + 1 == steps):
                if self._aa is not None:
                    row = self._aa.table[self.steps_done - 1].cpu()    # (synchronises)
                    rel = row[:, 0] / row[:, 1]
                else:
                    row = self.history[self.steps_done - 1].cpu()      # (synchronises)
                    rel = row[:, 4] / row[:, 5]
                if bool((rel < tol).all()):
                    break
        return self.history[:self.steps_done].cpu()

    def reset(self, x=None):
        """Back to step 0 from the initial node state (or from `x` [N,12], un-normalised); the history is cleared, the field
        statistics and the wall forces (if any) start over and the boundary data (if any) are those of step 1 again."""
        src = self._x0 if x is None else x
        if x is not None:
            require_gpu(x)
            if tuple(x.shape) != tuple(self.x_backup.shape):
                raise ValueError(f"x must be {tuple(self.x_backup.shape)}")
        self.x_backup.copy_(src)
        self.x.copy_(src)
        self.history.zero_()
        self._state.zero_()
        if self._aa is not None:
            self._aa.reset()
        for f in self._followers:
            f.reset()                                                          # (behind the counter's zero)
        self.steps_done = 0
        self._outs = None

    # ---- Anderson acceleration -----------------------------------------------------------------------------------------
    def _need_anderson(self):
        if self._aa is None:
            raise RuntimeError("this Rollout was built with anderson=0")
        return self._aa

    def anderson_history(self):
        """The acceleration's table so far as a CPU tensor [k, B, 4]: || G(x) - x ||_2, || G(x) ||_2, the depth used and the
        flags (gfv.anderson.NONFINITE / GROWTH / SINGULAR) per step and graph."""
        return self._need_anderson().table[:self.steps_done].cpu()

    def anderson_stats(self):
        """Restarts per graph (and the ring's state words); synchronises."""
        return self._need_anderson().stats()
