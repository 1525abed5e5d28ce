"""`gfv.optim.Adam` - torch.optim.Adam for users who change ONE import: the same constructor, `step()`, `zero_grad()`,
`param_groups` (so `torch.optim.lr_scheduler.*` drive it), `state_dict()` / `load_state_dict()` nesting - over flat fp32
buffers and the library's fused Adam launch (include/gfv.h gfv_adam_step_dev) instead of ~12 `_foreach_*` passes over 159
tensors (pre_train_Adam.py:79,191; solve_with_grad_GPU.py:181).

What it does to the model: the parameters become views of one flat buffer (16-byte aligned, in the order they were given - as
`gfv.trainer.TrainStep` lays them out); `NNmodel`'s backward hands out gradients as views of one flat tensor in the same
layout, which `step()` recognises and feeds to the kernel as it is (otherwise the gradients are gathered into a flat buffer
first: still one optimiser launch).  Parameter groups with their own `lr` and `weight_decay` (L2 as torch.optim.Adam,
decoupled as `AdamW` / `decoupled_weight_decay=True`) and the extra group key `"frozen": True` run inside the same launch
(gfv/groups.py, include/gfv.h gfv_adam_step_groups_dev); with one group, no decay and nothing frozen the launches are the ones
without groups.  Refused at construction: `amsgrad`, `maximize`, `differentiable`, groups whose `betas` or `eps` differ (the step
record is shared).  The step count is shared too: a parameter that starts to move after k steps (a group unfrozen, a `.grad` that
was None) continues with count k + 1 and zero moments, where torch, counting per parameter, starts its bias correction at 1.

`gfv.optim.LBFGS` - torch.optim.LBFGS for the closure loop of solve_with_grad_GPU_LBFGS.py:67-202, the same way: one import
changed, the same flat buffer, and the search direction in four launches (csrc/lbfgs.hip) instead of ~4 m launches and 2 m host
synchronisations of the two-loop recursion over history_size = m vectors.
"""
from __future__ import annotations

import torch

from . import lib as L
from .engine import GradStore
from .groups import MAX_GROUPS, ParamGroups, check_weight_decay
from .guard import GradGuard, check_policy
from .optstep import optimizer_launches


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False, grad_scale=1.0,
                 max_grad_norm=None, skip_nonfinite=False):
        check_policy(max_grad_norm)
        if amsgrad:
            raise NotImplementedError("gfv.optim.Adam: amsgrad=True needs a third moment buffer (the maximum of exp_avg_sq) the "
                                      "fused launch does not keep")
        if maximize:
            raise NotImplementedError("gfv.optim.Adam: maximize=True - the fused launch descends; negate the loss instead")
        if differentiable:
            raise NotImplementedError("gfv.optim.Adam: differentiable=True - the fused launch is not recorded by autograd")
        weight_decay = check_weight_decay(weight_decay)
        defaults = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                        weight_decay=0 if weight_decay == 0 else weight_decay, amsgrad=False, maximize=False)
        if decoupled_weight_decay:
            defaults["decoupled_weight_decay"] = True
        self._decoupled = bool(decoupled_weight_decay)
        super().__init__(params, defaults)
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"gfv.optim.Adam: {len(self.param_groups)} parameter groups, at most {MAX_GROUPS}")
        self._check_shared()
        ps = [p for g in self.param_groups for p in g["params"]]
        if not ps or any((not p.is_cuda) or p.dtype != torch.float32 for p in ps):
            raise RuntimeError("gfv.optim.Adam: fp32 parameters on the GPU (HIP kernels only, no CPU fallback)")
        dev = ps[0].device
        self._params = list(ps)
        self.G = GradStore([str(i) for i in range(len(ps))], [p.shape for p in ps], dev)
        total = self.G.total
        self.flat_g = self.G.flat
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(total, dtype=torch.float32, device=dev)
        self._offs = [self.G.off[str(i)] for i in range(len(ps))]
        self._adopt()
        self.adam_state = torch.zeros(16, dtype=torch.float32, device=dev)
        self.hyper = torch.zeros(8, dtype=torch.float32, device=dev)
        self._grad_scale = float(grad_scale)
        # training guard (gfv/guard.py): clip_grad_norm_ between backward() and step(), and "leave a non-finite step out", as two
        # launches inside step().  Every parameter is a segment: one whose `.grad` is None has zeros in its slots (below), which
        # add nothing to the norm - torch leaves it out
        self._guard = GradGuard(self.G, dev, max_grad_norm, skip_nonfinite)
        # parameter groups (gfv/groups.py): the tables exist from the first step that needs them
        # _stepped: positions that have state - loaded with some, or moved by a step (torch has no state for the others)
        self._pg, self._frozen_seen, self._stepped = None, None, set()
        self._hyper_host = None
        self._sync_hyper()
        L.status_mirror()   # the launch publishes the device status word (include/gfv.h gfv_status_mirror)

    # parameters as views of the flat buffer -------------------------------------------------------------------------
    def _adopt(self):
        for p, off in zip(self._params, self._offs):
            if p.data_ptr() != self.flat_p.data_ptr() + 4 * off:
                view = self.flat_p[off:off + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view

    def _sync_hyper(self, steps_done=None):
        g = self.param_groups[0]
        vals = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), self._grad_scale, 0.0, 0.0, 0.0)
        moved = self._hyper_host is None or vals[1:3] != self._hyper_host[1:3]
        if vals != self._hyper_host:
            self.hyper.copy_(torch.tensor(vals, dtype=torch.float32))
            self._hyper_host = vals
        if moved or steps_done is not None:
            t = float(self.adam_state[0]) if steps_done is None else float(steps_done)
            L.check(L.load().gfv_adam_state_init(self.adam_state.data_ptr(), float(g["betas"][0]), float(g["betas"][1]), t,
                                                 L.stream_ptr()), "adam_state_init")

    # parameter groups ------------------------------------------------------------------------------------------------
    def _check_shared(self):
        g0 = self.param_groups[0]
        for g in self.param_groups:
            for k in ("amsgrad", "maximize"):
                if g.get(k):
                    raise NotImplementedError(f"gfv.optim.Adam: a parameter group with {k}=True")
            if tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"]:
                raise NotImplementedError("gfv.optim.Adam: parameter groups with their own betas or eps - the step record (bias "
                                          "corrections, 1 - beta) is shared by all groups")

    def _groups_in_use(self):
        gs = self.param_groups
        return len(gs) > 1 or float(gs[0]["weight_decay"]) != 0.0 or bool(gs[0].get("frozen", False))

    def _sync_groups(self):
        """The tables follow param_groups (a scheduler edits "lr"; "weight_decay" and "frozen" may be edited too) and the set of
        parameters whose `.grad` is None this step: those must not move under a decay, as in torch - their runs point at the
        reserved frozen row, rewritten in place when the set changes."""
        self._check_shared()
        vals = [(float(g["lr"]), check_weight_decay(g["weight_decay"]), bool(g.get("frozen", False))) for g in self.param_groups]
        if all(fr for _, _, fr in vals):   # (checked before a table is touched)
            raise ValueError("gfv.optim.Adam: every parameter group is frozen: nothing left to optimise")
        owner = [k for k, g in enumerate(self.param_groups) for _ in g["params"]]   # group of every parameter, by position
        if self._pg is None:
            self._pg = ParamGroups(self.G, self._params[0].device, {str(i): k for i, k in enumerate(owner)}, vals, self._decoupled)
        self._pg.sync(vals, self._decoupled)
        frozen = tuple(fr for _, _, fr in vals)
        if frozen != self._frozen_seen:
            # the guard's norm covers what clip_grad_norm_ would see: no frozen group
            self._guard.set_segments(self.G, {str(i) for i, k in enumerate(owner) if frozen[k]})
            self._frozen_seen = frozen
        none = {i for i, p in enumerate(self._params) if p.grad is None}
        self._pg.set_rows(none)
        self._stepped |= {i for i, k in enumerate(owner) if not frozen[k] and i not in none}

    def _flat_grad(self):
        """The gradients as ONE flat tensor in this object's layout.  NNmodel's backward returns exactly that - views of one
        flat tensor (gfv/functions.py ModelFn.backward), which autograd keeps as `.grad` without copying: recognised by every
        gradient sitting at its offset of one storage of the right size - else gathered into a flat buffer first."""
        ps, offs = self._params, self._offs
        grads = [p.grad for p in ps]
        first = next((i for i, g in enumerate(grads) if g is not None), None)
        if first is None:
            return None
        g0 = grads[first]
        st = g0.untyped_storage()
        b0 = g0.data_ptr() - 4 * offs[first]
        if (g0.dtype == torch.float32 and st.data_ptr() == b0 and st.nbytes() >= 4 * self.G.total
                and all(g is not None and g.data_ptr() == b0 + 4 * o for g, o in zip(grads, offs) if g is not None)
                and self._none_grad_ok(grads)):
            return torch.empty(0, dtype=torch.float32, device=g0.device).set_(st, 0, (self.G.total,), (1,))
        flat = self.flat_g
        views, srcs = [], []
        for p, g, off in zip(ps, grads, offs):
            v = flat[off:off + p.numel()]
            if g is None:
                v.zero_()
            else:
                views.append(v.view(p.shape))
                srcs.append(g if g.dtype == torch.float32 else g.float())
        torch._foreach_copy_(views, srcs)
        return flat

    def _none_grad_ok(self, grads):
        """A parameter WITHOUT a gradient must keep its value (torch.optim.Adam skips it).  In NNmodel's flat gradient the slots of
        the parameters that never receive one (the unused ln_1 / Attn.temperature: gfv.functions.unused_param_names) hold zeros,
        which leaves m, v and the parameter as they are; any OTHER missing gradient (a layer frozen by `p.grad = None`) has a
        live value in its slot, so the flat tensor cannot be used as it is.  The backward says which slots are of the first kind
        (gfv.functions.LAST_FLAT: storage address + positions without a gradient)."""
        from . import functions as GF
        info = GF.LAST_FLAT
        none = frozenset(i for i, g in enumerate(grads) if g is None)
        first = next(g for g in grads if g is not None)
        return info is not None and info[0] == first.untyped_storage().data_ptr() and info[1] == none

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L.raise_on_status("gfv.optim.Adam.step")
        self._adopt()        # (a .to() / load_state_dict(assign=True) since the last step re-pointed the parameters)
        self._sync_hyper()   # lr_scheduler.step() edits param_groups[0]["lr"]
        g = self._flat_grad()
        if g is None:
            return loss
        if self._pg is not None or self._groups_in_use():
            self._sync_groups()
        elif len(self._stepped) != len(self._params):
            self._stepped = set(range(len(self._params)))   # (without groups every parameter takes part in the launch)
        optimizer_launches(self.flat_p, g, self.flat_m, self.flat_v, self.G.total, self.adam_state, self.hyper, guard=self._guard,
                           groups=self._pg)
        return loss

    max_grad_norm = property(lambda self: self._guard.max_grad_norm)
    skip_nonfinite = property(lambda self: self._guard.skip_nonfinite)

    @max_grad_norm.setter
    def max_grad_norm(self, v):
        check_policy(v)
        self._guard.set(v, self._guard.skip_nonfinite, False)

    @skip_nonfinite.setter
    def skip_nonfinite(self, v):
        self._guard.set(self._guard.max_grad_norm, v, False)

    def guard_stats(self):
        """As gfv.trainer.TrainStep.guard_stats (synchronises)."""
        return self._guard.stats()

    # torch.optim.Adam's checkpoint nesting (importer.py:292-313 stores it under `optimizer0`) ---------------------------
    def state_dict(self):
        t = self.adam_state[0:1].detach().cpu().clone().reshape(())
        state = {}
        for i, (p, off) in enumerate(zip(self._params, self._offs)):
            k = p.numel()
            if self._pg is not None and i not in self._stepped:
                continue   # (frozen, or never with a gradient: no state in torch either)
            state[i] = {"step": t.clone(), "exp_avg": self.flat_m[off:off + k].view(p.shape).detach().cpu().clone(),
                        "exp_avg_sq": self.flat_v[off:off + k].view(p.shape).detach().cpu().clone()}
        groups, at = [], 0
        for g in self.param_groups:
            group = {k: v for k, v in g.items() if k != "params"}
            group["params"] = list(range(at, at + len(g["params"])))
            at += len(g["params"])
            groups.append(group)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        if [len(g["params"]) for g in sd["param_groups"]] != [len(g["params"]) for g in self.param_groups]:
            raise ValueError("optimizer state belongs to a different parameter set")
        steps = {float(st["step"]) for st in sd["state"].values()}
        if len(steps) > 1:   # (checked before a buffer is touched)
            raise ValueError("per-parameter step counts differ: not a state this fused Adam can resume")
        step = steps.pop() if steps else None
        self.flat_m.zero_()
        self.flat_v.zero_()
        for i, st in sd["state"].items():
            i = int(i)
            off, k = self._offs[i], self._params[i].numel()
            self.flat_m[off:off + k].copy_(st["exp_avg"].reshape(-1))
            self.flat_v[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
        for mine, g in zip(self.param_groups, sd["param_groups"]):
            for k, v in g.items():
                if k != "params":
                    mine[k] = v
        self._stepped = {int(i) for i in sd["state"]}
        self._sync_hyper(steps_done=0.0 if step is None else step)


class AdamW(Adam):
    """torch.optim.AdamW on the fused launch: `Adam` with torch's AdamW defaults (weight_decay = 1e-2) and decoupled decay."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **kw):
        kw.pop("decoupled_weight_decay", None)
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, decoupled_weight_decay=True, **kw)


class LBFGS(torch.optim.Optimizer):
    """torch.optim.LBFGS with the same constructor, defaults, `step(closure)` semantics and checkpoint keys, on the library's
    L-BFGS launches (include/gfv.h gfv_lbfgs_*).

    Per iteration: pair, multidot, coef, combine - the two-loop recursion on coefficients over {s_i, y_i, g} with their dot
    products kept in double on the device (same gamma = ys / y.y, same skip rule ys > 1e-10) - then ONE read of a 128-byte
    result block; per closure evaluation: one masked copy + dot launch and ONE read (loss, g.d, max|g|, sum|g|).  Nothing on
    the host is proportional to history_size or to the number of parameters.  The strong-Wolfe search runs on host scalars
    (gfv/linesearch.py); the gradients of its live points stay in three device slots, and the point it returns hands its
    gradient on without another evaluation, as torch does.

    Padding is not data: the flat layout pads every tensor to 16 bytes and the padding of a flat gradient is undefined, so the
    gradient enters through a masked copy and every vector this object owns is zero there; the parameters' padding is never
    written.  A parameter whose `.grad` is None contributes zeros (torch's `_gather_flat_grad`).

    Memory: the history is 2 * (history_size + 1) * n * 4 bytes (955 MB for the 1.18 M parameters of the model at
    history_size = 100; torch's grows to 2 * history_size * n * 4), allocated ONCE at construction - the extra slot holds the
    candidate pair, so that a rejected one does not cost the oldest.

    Raises at construction: ValueError for more than one parameter group, history_size outside [1, 128] or a
    `line_search_fn` other than None / "strong_wolfe"; RuntimeError for parameters that are not fp32 on the GPU."""

    MAX_HISTORY = 128
    # the flat buffer of the parameters and the recognition of NNmodel's flat gradient are Adam's
    _adopt, _flat_grad, _none_grad_ok = Adam._adopt, Adam._flat_grad, Adam._none_grad_ok

    def __init__(self, params, lr=1, max_iter=20, max_eval=None, tolerance_grad=1e-7, tolerance_change=1e-9, history_size=100,
                 line_search_fn=None):
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if line_search_fn not in (None, "strong_wolfe"):
            raise ValueError("gfv.optim.LBFGS: line_search_fn is None or 'strong_wolfe'")
        if not 1 <= int(history_size) <= self.MAX_HISTORY:
            raise ValueError(f"gfv.optim.LBFGS: history_size in [1, {self.MAX_HISTORY}] (the coefficient launch is one workgroup)")
        if max_eval is None:
            max_eval = max_iter * 5 // 4
        defaults = dict(lr=lr, max_iter=max_iter, max_eval=max_eval, tolerance_grad=tolerance_grad,
                        tolerance_change=tolerance_change, history_size=int(history_size), line_search_fn=line_search_fn)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("gfv.optim.LBFGS doesn't support per-parameter options (parameter groups)")
        ps = self.param_groups[0]["params"]
        if not ps or any((not p.is_cuda) or p.dtype != torch.float32 for p in ps):
            raise RuntimeError("gfv.optim.LBFGS: fp32 parameters on the GPU (HIP kernels only, no CPU fallback)")
        dev = ps[0].device
        self._params = list(ps)
        self.G = GradStore([str(i) for i in range(len(ps))], [p.shape for p in ps], dev)
        n = self.n = self.G.total
        self.flat_g = self.G.flat
        self.flat_p = torch.zeros(n, dtype=torch.float32, device=dev)
        self._offs = [self.G.off[str(i)] for i in range(len(ps))]
        self._adopt()
        mask = torch.zeros(n, dtype=torch.uint8)
        for p, off in zip(self._params, self._offs):
            mask[off:off + p.numel()] = 1
        self._idx = torch.nonzero(mask).reshape(-1).to(dev)   # flat position of every real element, in parameter order
        self.mask = mask.to(dev)
        self.slots = int(history_size) + 1
        self.R = 2 * self.slots + 1
        self.S = torch.zeros(self.slots * n, dtype=torch.float32, device=dev)
        self.Y = torch.zeros(self.slots * n, dtype=torch.float32, device=dev)
        self.gbuf = torch.zeros(3, n, dtype=torch.float32, device=dev)   # the current gradient + the line search's live points
        self._gcur = 0
        self.g_prev = torch.zeros(n, dtype=torch.float32, device=dev)
        self.d = torch.zeros(n, dtype=torch.float32, device=dev)
        self.x0 = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ring = torch.zeros(8, dtype=torch.int32, device=dev)        # head, count, accepted, -, arrival counter of dot
        self.M = torch.zeros(self.R * self.R, dtype=torch.float64, device=dev)
        self.delta = torch.zeros(self.R, dtype=torch.float64, device=dev)
        self.res = torch.zeros(16, dtype=torch.float64, device=dev)
        self.res[4] = 1.0
        ws = int(L.load().gfv_lbfgs_workspace_doubles(self.slots, n))
        if ws <= 0:
            raise RuntimeError("gfv.optim.LBFGS: the library refuses this size")
        self.partial = torch.zeros(ws, dtype=torch.float64, device=dev)
        self.dot_ws = torch.zeros(3 * (ws // (3 * self.R + 2)), dtype=torch.float64, device=dev)
        self.dot_out = torch.zeros(4, dtype=torch.float64, device=dev)   # g.d, max|g|, sum|g|, loss
        L.status_mirror()

    # launches -------------------------------------------------------------------------------------------------------
    def _ingest(self, g, slot):
        """Masked copy of the flat gradient `g` into slot `slot` + its dot with d, max|.|, sum|.| -> dot_out[0:3]."""
        L.check(L.load().gfv_lbfgs_dot(g.data_ptr(), self.mask.data_ptr(), self.gbuf[slot].data_ptr(), self.d.data_ptr(), self.n,
                                       self.dot_ws.data_ptr(), self.ring.data_ptr() + 16, self.dot_out.data_ptr(), L.stream_ptr()),
                "lbfgs_dot")

    def _evaluate(self, closure, slot):
        """One closure evaluation: (loss as returned, loss, g.d, max|g|, sum|g|), the gradient in slot `slot`.  One read."""
        with torch.enable_grad():
            orig = closure()
        g = self._flat_grad()
        if g is None:
            raise RuntimeError("gfv.optim.LBFGS: the closure left no gradient on any parameter")
        self._ingest(g, slot)
        if torch.is_tensor(orig) and orig.is_cuda:
            self.dot_out[3:4].copy_(orig.detach().reshape(1))
            r = self.dot_out.tolist()
        else:
            r = self.dot_out.tolist()
            r[3] = float(orig)
        return orig, r[3], r[0], r[1], r[2]

    def _direction(self, t, mode):
        """The four launches of a search direction from the gradient in the current slot; (g.d, max|d|, result block)."""
        lib, st = L.load(), L.stream_ptr()
        S, Y, g, ring = self.S.data_ptr(), self.Y.data_ptr(), self.gbuf[self._gcur].data_ptr(), self.ring.data_ptr()
        L.check(lib.gfv_lbfgs_pair(S, Y, self.slots, self.n, ring, g, self.g_prev.data_ptr(), self.d.data_ptr(), float(t),
                                   1 if mode == 1 else 0, st), "lbfgs_pair")
        L.check(lib.gfv_lbfgs_multidot(S, Y, self.slots, self.n, ring, g, self.partial.data_ptr(), mode, st), "lbfgs_multidot")
        L.check(lib.gfv_lbfgs_coef(ring, self.M.data_ptr(), self.partial.data_ptr(), self.delta.data_ptr(), self.res.data_ptr(),
                                   self.slots, self.n, mode, st), "lbfgs_coef")
        L.check(lib.gfv_lbfgs_combine(S, Y, self.slots, self.n, ring, g, self.delta.data_ptr(), self.d.data_ptr(),
                                      self.res.data_ptr(), st), "lbfgs_combine")
        r = self.res.cpu()
        return float(r[0]), float(r[8:9].view(torch.float32)[0]), r

    def _move(self, x0, t):
        L.check(L.load().gfv_lbfgs_axpy(self.flat_p.data_ptr(), x0.data_ptr(), self.d.data_ptr(), float(t), self.mask.data_ptr(),
                                        self.n, L.stream_ptr()), "lbfgs_axpy")

    @torch.no_grad()
    def step(self, closure):
        from .linesearch import strong_wolfe
        L.raise_on_status("gfv.optim.LBFGS.step")
        self._adopt()
        group = self.param_groups[0]
        lr = float(group["lr"])
        max_iter, max_eval = group["max_iter"], group["max_eval"]
        tolerance_grad, tolerance_change = group["tolerance_grad"], group["tolerance_change"]
        line_search_fn = group["line_search_fn"]
        if line_search_fn not in (None, "strong_wolfe"):
            raise RuntimeError("only 'strong_wolfe' is supported")
        state = self.state[self._params[0]]
        state.setdefault("func_evals", 0)
        state.setdefault("n_iter", 0)

        orig_loss, loss, _, gmax, gl1 = self._evaluate(closure, self._gcur)
        current_evals = 1
        state["func_evals"] += 1
        if gmax <= tolerance_grad:
            return orig_loss

        t = state.get("t")
        n_iter = 0
        while n_iter < max_iter:
            n_iter += 1
            state["n_iter"] += 1
            first = state["n_iter"] == 1
            gtd, dmax, _ = self._direction(0.0 if first else t, 1 if first else 0)
            state["prev_loss"] = prev_loss = loss
            if first:
                t = float(torch.tensor(min(1.0, 1.0 / gl1), dtype=torch.float32)) * lr   # (torch holds it in fp32)
            else:
                t = lr
            state["t"] = t
            if gtd > -tolerance_change:
                break

            ls_func_evals = 0
            opt_cond = False
            if line_search_fn is not None:
                self.x0.copy_(self.flat_p)
                slot_of, gmax_of, live = {0.0: self._gcur}, {0.0: gmax}, [(0.0,)]

                def keep(ts):
                    live[0] = ts

                def phi(tt):
                    used = {slot_of[x] for x in live[0] if x in slot_of}
                    slot = next(s for s in range(3) if s not in used)
                    for key in [key for key, v in slot_of.items() if v == slot]:
                        del slot_of[key]
                    self._move(self.x0, tt)
                    _, f, gtd_new, gm, _ = self._evaluate(closure, slot)
                    slot_of[tt], gmax_of[tt] = slot, gm
                    return f, gtd_new

                # (tolerance_change of the search is its default, as in torch's call)
                loss, t, ls_func_evals = strong_wolfe(phi, t, loss, gtd, max_ls=max_eval - current_evals, d_norm=dmax, keep=keep)
                self._gcur, gmax = slot_of[t], gmax_of[t]
                self._move(self.x0, t)
                state["t"] = t
                opt_cond = gmax <= tolerance_grad
            else:
                self._move(self.flat_p, t)
                if n_iter != max_iter:
                    _, loss, _, gmax, _ = self._evaluate(closure, self._gcur)
                    opt_cond = gmax <= tolerance_grad
                    ls_func_evals = 1

            current_evals += ls_func_evals
            state["func_evals"] += ls_func_evals

            if n_iter == max_iter:
                break
            if current_evals >= max_eval:
                break
            if opt_cond:
                break
            if dmax * abs(t) <= tolerance_change:
                break
            if abs(loss - prev_loss) < tolerance_change:
                break
        return orig_loss

    # torch.optim.LBFGS's checkpoint: everything under state[0] (importer.py stores it under `optimizer0`) --------------------
    def _unpadded(self, v):
        return v[self._idx].detach().cpu().clone()

    def _padded(self, dst, v):
        dst.zero_()
        dst[self._idx] = v.detach().to(device=dst.device, dtype=torch.float32).reshape(-1)

    def state_dict(self):
        state = self.state.get(self._params[0], {})
        out = {k: state[k] for k in ("func_evals", "n_iter") if k in state}
        if state.get("n_iter", 0) >= 1:
            n, m1, R = self.n, self.slots, self.R
            ring = self.ring.cpu()
            head, count = int(ring[0]), int(ring[1])
            M = self.M.view(R, R).cpu()
            slots = [(head + i) % m1 for i in range(count)]
            out["d"] = self._unpadded(self.d)
            out["t"] = state["t"]
            out["old_dirs"] = [self._unpadded(self.Y[s * n:(s + 1) * n]) for s in slots]
            out["old_stps"] = [self._unpadded(self.S[s * n:(s + 1) * n]) for s in slots]
            out["ro"] = [(1.0 / M[s, m1 + s]).clone() for s in slots]
            out["H_diag"] = self.res[4].detach().cpu().clone()
            out["prev_flat_grad"] = self._unpadded(self.g_prev)
            out["prev_loss"] = state["prev_loss"]
            out["al"] = [None] * self.param_groups[0]["history_size"]
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self._params)))
        return {"state": {0: out} if out else {}, "param_groups": [group]}

    def load_state_dict(self, sd):
        g = sd["param_groups"][0]
        if len(sd["param_groups"]) != 1 or len(g["params"]) != len(self._params):
            raise ValueError("optimizer state belongs to a different parameter set")
        src = {int(k): v for k, v in sd["state"].items()}.get(0, {})
        for k, v in g.items():
            if k not in ("params", "history_size"):   # (the ring was sized at construction)
                self.param_groups[0][k] = v
        state = self.state[self._params[0]]
        state.clear()
        for k in ("func_evals", "n_iter", "prev_loss"):
            if k in src:
                state[k] = src[k]
        n, m1 = self.n, self.slots
        self.ring.zero_()
        self.M.zero_()
        self.res.zero_()
        H = src.get("H_diag", 1.0)
        self.res[4] = float(H)
        if "t" in src:
            state["t"] = float(src["t"])
        if "d" in src:
            self._padded(self.d, src["d"])
        if "prev_flat_grad" in src and src["prev_flat_grad"] is not None:
            self._padded(self.g_prev, src["prev_flat_grad"])
        dirs, stps = list(src.get("old_dirs", [])), list(src.get("old_stps", []))
        if len(dirs) != len(stps):
            raise ValueError("old_dirs and old_stps differ in length")
        dirs, stps = dirs[-(m1 - 1):], stps[-(m1 - 1):]
        lib, st = L.load(), L.stream_ptr()
        for i, (y, s) in enumerate(zip(dirs, stps)):
            self._padded(self.Y[i * n:(i + 1) * n], y)
            self._padded(self.S[i * n:(i + 1) * n], s)
            # the pair's rows of the dot-product matrix, by the launches that wrote them the first time: the same bits
            L.check(lib.gfv_lbfgs_multidot(self.S.data_ptr(), self.Y.data_ptr(), m1, n, self.ring.data_ptr(),
                                           self.gbuf[self._gcur].data_ptr(), self.partial.data_ptr(), 2, st), "lbfgs_multidot")
            L.check(lib.gfv_lbfgs_coef(self.ring.data_ptr(), self.M.data_ptr(), self.partial.data_ptr(), self.delta.data_ptr(),
                                       self.res.data_ptr(), m1, n, 2, st), "lbfgs_coef")
