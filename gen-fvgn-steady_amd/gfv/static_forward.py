"""The forward-only step on static weight images, for whoever runs a model that is not being trained (`Rollout`, `Sweep`,
`Evaluate`): `Engine.forward` with keep=False and static weights - the launches of the training forward on the same kernel families,
with NULL for every tensor only a backward would read, bit-identical outputs - on weight images built ONCE, in the constructor and
in `refresh()`, not per step.  What a recorded list of such a step points at, and who owns it, is DESIGN.md 5l.
"""
from __future__ import annotations

import contextlib
import weakref

import torch

from . import lib as L

_PADDED = weakref.WeakKeyDictionary()       # engine -> the padded copies of its (narrow) model's parameters


def check_normalizer(model):
    """For the users that run batch after batch of a pool (`Sweep`, `Evaluate`; the message is the one both have always given)."""
    if model.node_norm.should_accumulate():
        raise ValueError("Sweep: the model's Normalizer is still accumulating; its statistics would couple the graphs of a "
                         "batch, so an entry's result would depend on its neighbours.  Sweep a trained model")


def prep_scratch(max_graphs, dev):
    """-> (_prep_ws, _fvm_cnt): the engine scratch of the input preparation and of the finite-volume tail for batches of up to
    `max_graphs` graphs.  Whoever records lists creates it once and never reallocates it."""
    words = max(L.load().gfv_prep_workspace_bytes(max_graphs) // 4, 1)
    return torch.zeros(words, dtype=torch.float32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)


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


class StaticForward:
    """Owns `P` (a narrow model: the padded copies), the Normalizer `buffers`, the `WeightGuard`, the engine scratch of the input
    preparation and of the finite-volume tail sized for `max_graphs` (created once, never reallocated) and the signature of what
    a recorded list points at outside its own pool."""

    def __init__(self, model, max_graphs, dev):
        self.model, self.engine = model, model.engine()
        self._prep_ws, self._fvm_cnt = prep_scratch(max_graphs, dev)
        # name -> padded copy of a narrow model's parameter; one set per engine, as a full-width model's own tensors are: every
        # runner of a model then names ONE parameter set to the engine, and they can take turns on it
        self._padded = _PADDED.setdefault(self.engine, {})
        self.guard = WeightGuard(model)
        self.sig = None
        self.refresh()

    def signature(self):
        """The parts of Engine.capture_signature() a forward-only list depends on - the parameter set the image set belongs to,
        the product form, and the image set itself (images are added to a set, never moved; the descriptor table of the per-step
        rebuild is not part of a list that builds no images) - and the addresses of the parameters (a narrow model: of their
        padded copies) and buffers."""
        sig, wi = self.engine.capture_signature(), self.engine._wi
        return ((sig[0], sig[2], None if wi is None else id(wi["fwd"])), tuple(t.data_ptr() for t in self.P.values()),
                tuple(b.data_ptr() for b in self.buffers.values()))

    def refresh(self):
        """(Re)build what depends on the parameter VALUES, in place: padded copies (hidden_size < 128) by `copy_` into the tensors
        that exist, the maximum and every forward weight image into the memory they have, on the calling stream.  -> whether
        something a recorded list points at moved (its owner then has to drop its lists)."""
        from FVMmodel.padding import pad_parameters
        names, tensors = self.model.param_names_tensors()
        P = {}
        with torch.no_grad():
            for name, src, t in zip(names, tensors, pad_parameters(names, tensors, self.model.hidden_size)):
                if t is src:
                    P[name] = src.detach()
                    continue
                own = self._padded.get(name)
                if own is not None and own.shape == t.shape and own.device == t.device:
                    own.copy_(t)
                else:
                    own = self._padded[name] = t.detach()
                P[name] = own
        self.P = P
        self.buffers = self.model.node_norm.buffers_dict()
        self.model.node_norm._host_num_acc = None
        with self.engine.model_width():
            # (same parameter set - same addresses: the maximum and EVERY known image are rebuilt where they are; another one:
            # the engine starts a new image set, and the signature below says so)
            self.engine.build_static_images(P)
        self.guard.refresh()
        old, self.sig = self.sig, self.signature()
        return self.sig != old

    def check(self, who, run):
        """Raises instead of letting stale images be used: after `load_state_dict`, an optimizer step, `.to()` or another
        parameter set through the same engine, `refresh()` comes first."""
        self.guard.check()
        if self.signature() != self.sig:
            raise RuntimeError(f"{who}: the engine's weight-image set changed under the {run} (another parameter set or product "
                               "form went through the same engine); call refresh_weights()")

    @contextlib.contextmanager
    def _own_scratch(self):
        """The engine works on this object's scratch for the duration of a step, so that another batch run through the same
        engine cannot replace what a recorded list points at."""
        eng = self.engine
        saved = (eng._prep_ws, eng._fvm_cnt)
        eng._prep_ws, eng._fvm_cnt = self._prep_ws, self._fvm_cnt
        try:
            yield
        finally:
            assert eng._prep_ws is self._prep_ws and eng._fvm_cnt is self._fvm_cnt, "engine scratch was reallocated inside a step"
            eng._prep_ws, eng._fvm_cnt = saved

    def forward(self, x, x_raw, pl, accumulate, norm_global):
        """-> (losses [B,4], uvp_node [N,3], uvp_cell [C,3]) of the batch `pl` describes; nothing is saved for a backward."""
        with self._own_scratch(), self.engine.model_width():
            losses, uvp_node, uvp_cell, _, sv = self.engine.forward(
                self.P, self.buffers, x, pl, norm_global=norm_global, accumulate=accumulate, want_outputs=True,
                want_edge_attr15=False, x_raw=x_raw, keep=False, static_weights=True)
        assert sv is None
        return losses, uvp_node, uvp_cell
