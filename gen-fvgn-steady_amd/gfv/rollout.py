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

Who owns what a recorded list points at.  The list's own allocations (activations, outputs) live in the private memory pool of
the `CommandList`; inside it the forward frees and re-uses blocks, which is correct in stream order because the forward-only
step issues every launch on ONE stream (its weight images are static: no side-stream build, no fork).  Everything else the list
reads is created in set-up and held by this object for its lifetime, never reallocated: `x`, `x_backup`, the history, the step
counter, the reduction workspace, the engine scratch of the input preparation and of the finite-volume tail (swapped into the
engine for the duration of a step, so that another batch run through the same engine cannot replace them), the padded
parameters of a narrow model, the plan and the graphs.  The weight images belong to the engine's image set of this parameter
set, which the engine keeps (also after it has been superseded).

Weights.  Images (and, for hidden_size < 128, the padded copies) are built ONCE - in the constructor and in
`refresh_weights()` - not per step: the parameters of a model that is being run do not change.  Each `step()` compares the
parameters' storage and in-place version counters and the parts of `Engine.capture_signature()` a forward-only list depends on
(parameter set, product form, identity of the image set) with what the images were built for and raises on a mismatch instead
of replaying stale images: after `load_state_dict`, an optimizer step or `.to()`, call `refresh_weights()`.

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
"""
from __future__ import annotations

import contextlib

import torch

from . import anderson as AA
from . import cmdlist
from . import lib as L
from .functions import require_gpu
from .plan import get_plan

HISTORY_WIDTH = 6   # (loss_cont, loss_mom_x, loss_mom_y, loss_press, ||uvp_new - uvp_prev||_2, ||uvp_new||_2) per graph


def check_room(steps_done, max_steps, steps=1):
    """The history holds `max_steps` rows: a step that would write past it is refused on the host (the kernel would skip the
    row, but the caller asked for a record of every step)."""
    if steps_done + steps > max_steps:
        raise IndexError(f"Rollout: {steps_done} steps done + {steps} asked for exceeds max_steps={max_steps} "
                         "(the device history has one row per step); reset() or build the Rollout with a larger max_steps")


class WeightGuard:
    """What the weight images of a Rollout were built for: the storage and in-place version of every parameter and Normalizer
    buffer location.  `check()` raises when any of them changed since `refresh()`."""

    def __init__(self, model):
        self.model = model
        self.sig = None
        self.refresh()

    def signature(self):
        _, tensors = self.model.param_names_tensors()
        return (tuple(t._version for t in tensors), tuple(t.data_ptr() for t in tensors),
                tuple(b.data_ptr() for b in self.model.node_norm.buffers_dict().values()))

    def refresh(self):
        self.sig = self.signature()

    def check(self):
        if self.signature() != self.sig:
            raise RuntimeError("Rollout: the model's parameters changed (load_state_dict, an optimizer step, .to()) since the "
                               "weight images were built; call refresh_weights() before the next step")


class Rollout:
    WARM = 2   # eager steps before a list is recorded (they are steps of the rollout like any other)

    def __init__(self, model, graphs, max_steps=1000, launch_mode="cmd_list", norm_global=None, anderson=0, anderson_beta=1.0,
                 anderson_reg=1e-10, anderson_restart=10.0, anderson_start=0):
        if launch_mode not in ("cmd_list", "eager"):
            raise ValueError('launch_mode must be "cmd_list" or "eager"')
        aa_args = AA.check_args(anderson, anderson_beta, anderson_reg, anderson_restart, anderson_start)
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
        lib = L.load()
        self._prep_ws = torch.zeros(max(lib.gfv_prep_workspace_bytes(pl.B) // 4, 1), dtype=torch.float32, device=dev)
        self._fvm_cnt = torch.zeros(4, dtype=torch.int32, device=dev)
        L.status_mirror()
        self.anderson = aa_args[0]
        self._aa = AA.AndersonState(pl, dev, self.max_steps, *aa_args) if self.anderson else None
        self.steps_done = 0
        self._lists, self._warm = {}, {}
        self._outs = None
        self._guard = WeightGuard(model)
        self.refresh_weights()

    # ---- weights -------------------------------------------------------------------------------------------------------
    def refresh_weights(self):
        """(Re)build what depends on the parameter VALUES: padded copies (hidden_size < 128) and the forward weight images.
        Recorded lists are dropped (the next steps warm up and record again)."""
        from FVMmodel.padding import pad_parameters
        names, tensors = self.model.param_names_tensors()
        with torch.no_grad():
            padded = pad_parameters(names, tensors, self.model.hidden_size)
            self.P = dict(zip(names, (t.detach() for t in padded)))
        self.buffers = self.model.node_norm.buffers_dict()
        self.model.node_norm._host_num_acc = None
        self._lists, self._warm = {}, {}
        with self.engine.model_width():
            self.engine.build_static_images(self.P)
        self._guard.refresh()
        self._sig = self._engine_signature()

    def _engine_signature(self):
        """The parts of Engine.capture_signature() a forward-only list depends on: the parameter set the image set belongs to,
        the product form, and the image set itself (images are added to a set, never moved; the descriptor table of the per-step
        rebuild is not part of a list that builds no images)."""
        sig = self.engine.capture_signature()
        wi = self.engine._wi
        return (sig[0], sig[2], None if wi is None else id(wi["fwd"]))

    # ---- one step ------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _own_scratch(self):
        eng = self.engine
        saved = (eng._prep_ws, eng._fvm_cnt)
        eng._prep_ws, eng._fvm_cnt = self._prep_ws, self._fvm_cnt
        try:
            yield
        finally:
            assert eng._prep_ws is self._prep_ws and eng._fvm_cnt is self._fvm_cnt, "engine scratch was reallocated inside a step"
            eng._prep_ws, eng._fvm_cnt = saved

    def _body(self, acc):
        pl = self.plan
        with self._own_scratch(), self.engine.model_width():
            losses, uvp_node, uvp_cell, _, sv = self.engine.forward(
                self.P, self.buffers, self.x, pl, norm_global=self.norm_global, accumulate=acc, want_outputs=True,
                want_edge_attr15=False, x_raw=self.x_backup, keep=False, static_weights=True)
        assert sv is None
        if self._aa is not None:
            self._aa.launch(uvp_node, self.x_backup, self._state)
        L.check(L.load().gfv_rollout_advance(
            uvp_node.data_ptr(), self.x_backup.data_ptr(), self.x.data_ptr(), pl.N, pl.chunk_beg.data_ptr(),
            pl.chunk_end.data_ptr(), pl.gchunk_ptr.data_ptr(), pl.n_chunks, pl.B, losses.data_ptr(), self._partial.data_ptr(),
            self.history.data_ptr(), self.max_steps, self._state.data_ptr(), L.stream_ptr()), "gfv_rollout_advance")
        L.status_publish()
        return losses, uvp_node, uvp_cell

    def step(self):
        """One forward-only step + advance -> (losses [B,4], uvp_node [N,3], uvp_cell [C,3]).  In list mode the three are the
        recorded step's own tensors: the next step overwrites them.  With `anderson` > 0 uvp_node is the iterate the rollout
        advanced to (the mixed one where the step was accelerated)."""
        L.raise_on_status("Rollout.step")
        check_room(self.steps_done, self.max_steps)
        self._guard.check()
        if self._engine_signature() != self._sig:
            raise RuntimeError("Rollout: the engine's weight-image set changed under the rollout (another parameter set or product "
                               "form went through the same engine); call refresh_weights()")
        norm = self.model.node_norm
        acc = self.norm_global and norm.should_accumulate()
        if self.launch_mode == "eager" or cmdlist.active() is not None or torch.cuda.is_current_stream_capturing():
            outs = self._body(acc)
        else:
            ent = self._lists.get(acc)
            if ent is not None:
                ent[0].replay()
                outs = ent[1]
            elif self._warm.get(acc, 0) < Rollout.WARM:
                self._warm[acc] = self._warm.get(acc, 0) + 1
                outs = self._body(acc)
            else:
                with cmdlist.record() as cl:
                    outs = self._body(acc)
                self._lists[acc] = (cl, outs)
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
        """Back to step 0 from the initial node state (or from `x` [N,12], un-normalised); the history is cleared."""
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
