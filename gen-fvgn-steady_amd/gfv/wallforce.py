"""Wall forces: the drag, lift and moment history of a run, summed on the device.

A cylinder or airfoil run is made for the force on the body: the drag and lift history, the mean drag, the r.m.s. lift, the
shedding frequency from the lift signal.  `Rollout` and `MarchStep` exist so that the host never synchronises per step;
`WallForces` is two small launches behind the launch that advances the field (`gfv_wall_force_grad`, `gfv_wall_force_sum`;
csrc/wallforce.hip, include/gfv.h), following the owner's clock - `Rollout`'s step counter, `MarchStep`'s level count - the way
`FieldStats` does (gfv/follow.py), sampling the fields of the same window rule (gfv/window.py):

    wf = WallForces(box=(0.05, 0.35, 0.08, 0.32), origin=(0.2, 0.2), start=1, stride=1, stop=None, keep=4096)
    r = Rollout(model, graphs, max_steps=2000, wall_forces=wf)
    r.run(steps=2000)
    h = wf.read()                          # n, clock [k], pressure [k,B,2], viscous [k,B,2], moment [k,B,2], faces [B]
    c = wf.coefficients(ref_length=0.1, ref_speed=1.0)       # cd, cl, cm [k,B]
    ms = MarchStep(model, graphs, ..., wall_forces=WallForces(box=...))     # one sample per completed level
    f = evaluate(graphs, field, box=..., origin=...)         # one shot, no owner -> [B, 6] float64

What the force is.  The momentum flux that the residual itself attributes to the wall faces (the P_flux - vis_flux of
FVscheme.py:203-229), per graph, dimensionless, in the units of the residual, for the field `x_backup[:, 0:3]` as the advance
launch has just written it: node values divided by `uvp_dim` (one fp32 division), node gradients by the WLSQ reconstruction of the
plan's order kept in double, face values as the face kernel forms them, and per selected face with its one incidence's surface
vector S (the cell's outward vector: it points into the body)

    Fp = theta3 * p_f * S        Fv[c] = -theta4 * (G_f[c] . S)        M = arm x F,  arm = face centre - origin

`Fp + Fv` is the force of the fluid ON THE WALL.  The convective flux is left out: it is zero on a wall whose velocity has no
normal component (a body that moves through its own surface is not covered).  theta3 and theta4 are read from the plan's
device tensor at every launch.  The rule in full: include/gfv.h.

Which faces.  A face qualifies if its type is WALL_BOUNDARY and it has exactly ONE (cell, face) incidence - an interior edge
between two wall nodes carries the wall type too, has two, and is never selected (named explicitly it is refused).  `faces`
(a bool [E] mask or an integer index tensor) and `box` = (xmin, xmax, ymin, ymax) on the face centre (or a list of B boxes, one per
graph) narrow the selection; with both, both must hold.  A graph may end up with no face (its rows are zero); no face at all is
refused.  The selection is fixed when the owner attaches the object: a later edit of `face_type` does not move it.  Selection and
tables are plain torch ops that need no GPU: `select_faces`, `build_tables`.

The ring holds the last `keep` samples; the time of a sample is joined through its clock (`Rollout`: clock * dt; a `MarchStep`
with a `StepControl`: `step_history()`).  No floating-point atomics, no sum across graphs, a fixed summation order: the same run
gives the same bits.

Who owns what a recorded list points at: DESIGN.md 5l.  Particular to this object, allocated once when its owner attaches it and
never reallocated: the record, the tables, the gradients of the body nodes, the partial sums, the ring and its clocks, the origin.
One owner per object.  The forces are not part of any `state_dict()`.
"""
from __future__ import annotations

import numbers

import torch

from . import lib as L
from .fieldstats import check_field
from .follow import Follower
from .window import N_SAMPLES, UNCHANGED, Window

WALL_BOUNDARY = 3
TERMS = (2, 5, 9, 14)


# ---- checks that need no GPU -----------------------------------------------------------------------------------------------------
def check_keep(keep):
    if isinstance(keep, bool) or not isinstance(keep, numbers.Integral) or not 1 <= keep < 2 ** 31:
        raise ValueError(f"keep must be an integer in 1 .. 2^31 - 1 (rows of the ring), got {keep!r}")
    return int(keep)


def _is_number(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def check_box(box, B=None):
    """None, one (xmin, xmax, ymin, ymax) or a list of B of them -> None or a list of 4-tuples of floats (one: for every graph)."""
    if box is None:
        return None
    try:
        items = list(box)
    except TypeError:
        raise ValueError(f"box must be (xmin, xmax, ymin, ymax) or a list of such, got {box!r}") from None
    single = len(items) == 4 and all(_is_number(v) for v in items)
    boxes = [items] if single else items
    out = []
    for bx in boxes:
        try:
            vals = list(bx)
        except TypeError:
            raise ValueError(f"box must be (xmin, xmax, ymin, ymax) or a list of such, got {box!r}") from None
        if len(vals) != 4 or not all(_is_number(v) for v in vals):
            raise ValueError(f"a box is four numbers (xmin, xmax, ymin, ymax), got {bx!r}")
        vals = tuple(float(v) for v in vals)
        if not (vals[0] <= vals[1] and vals[2] <= vals[3]):          # (a NaN fails this too)
            raise ValueError(f"a box needs xmin <= xmax and ymin <= ymax, got {bx!r}")
        out.append(vals)
    if not out:
        raise ValueError("box: an empty list")
    if B is not None and not single and len(out) != B:
        raise ValueError(f"box: a list gives one box per graph: {len(out)} boxes for {B} graphs")
    return out


def check_origin(origin, B=None):
    """(x, y) or a list of B pairs -> a list of pairs of floats (one: for every graph)."""
    try:
        items = list(origin)
    except TypeError:
        raise ValueError(f"origin must be (x, y) or a list of such, got {origin!r}") from None
    single = len(items) == 2 and all(_is_number(v) for v in items)
    pairs = [items] if single else items
    out = []
    for pr in pairs:
        try:
            vals = list(pr)
        except TypeError:
            raise ValueError(f"origin must be (x, y) or a list of such, got {origin!r}") from None
        if len(vals) != 2 or not all(_is_number(v) and v == v and abs(v) != float("inf") for v in vals):
            raise ValueError(f"an origin is two finite numbers (x, y), got {pr!r}")
        out.append((float(vals[0]), float(vals[1])))
    if not out:
        raise ValueError("origin: an empty list")
    if B is not None and not single and len(out) != B:
        raise ValueError(f"origin: a list gives one point per graph: {len(out)} points for {B} graphs")
    return out


def check_graphs(graphs):
    """Batches of a DevicePool are refused (the pool rewrites their face types and coefficients between batches; a selection fixed
    at attach time would not follow it).  Needs no GPU."""
    if getattr(graphs[0], "_gfv_pool_plan", None) is not None:
        raise ValueError("WallForces: graphs of a DevicePool are not supported (the pool owns their face types and coefficients; "
                         "Sweep and PoolTrainStep are out of scope)")


def check_owner(who, wall_forces, graphs=None, anderson=0):
    """What an owner refuses of `wall_forces=`; needs no GPU."""
    WallForces.check_handed(who, wall_forces, graphs, anderson)


# ---- selection and tables: plain torch ops on whatever device the graphs live on ----------------------------------------------
def face_graph(graphs):
    """The graph of every face [E] (int64): that of its first end node."""
    gn = graphs[0]
    return gn.batch.reshape(-1)[gn.edge_index[0]].to(torch.int64)


def select_faces(graphs, faces=None, box=None):
    """The selected faces as ascending int64 indices [Nf] (on the graphs' device).  Qualifying: face_type == WALL_BOUNDARY and
    exactly one (cell, face) incidence; `faces` (bool [E] mask or integer indices) must name qualifying faces only; `box` keeps
    the faces whose centre lies inside (bounds included).  ValueError when nothing is left."""
    ge = graphs[2]
    ftype = ge.face_type.reshape(-1)
    E = int(ftype.shape[0])
    B = int(graphs[4].theta_PDE.shape[0])
    dev = ftype.device
    inc = torch.bincount(ge.face.reshape(-1).to(torch.int64), minlength=E)
    ok = (ftype == WALL_BOUNDARY) & (inc == 1)
    sel = ok.clone()
    if faces is not None:
        if not isinstance(faces, torch.Tensor):
            faces = torch.as_tensor(faces)
        faces = faces.to(dev)
        if faces.dtype == torch.bool:
            if tuple(faces.shape) != (E,):
                raise ValueError(f"faces: a bool mask has one entry per face ({E}), got shape {tuple(faces.shape)}")
            named = faces
        elif faces.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            idx = faces.reshape(-1).to(torch.int64)
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= E):
                raise ValueError(f"faces: an index outside 0 .. {E - 1}")
            named = torch.zeros(E, dtype=torch.bool, device=dev)
            named[idx] = True
        else:
            raise ValueError(f"faces must be a bool [E] mask or an integer index tensor, got dtype {faces.dtype}")
        bad = named & ~ok
        if bool(bad.any()):
            f = int(torch.nonzero(bad)[0])
            why = ("is not a wall face" if int(ftype[f]) != WALL_BOUNDARY else
                   f"has {int(inc[f])} incidences (an interior edge between two wall nodes, not a face of the body's surface)")
            raise ValueError(f"faces: {int(bad.sum())} named faces do not qualify; face {f} {why}")
        sel = sel & named
    boxes = check_box(box, B)
    if boxes is not None:
        fb = face_graph(graphs)
        bt = torch.tensor(boxes if len(boxes) > 1 else boxes * B, dtype=torch.float64, device=dev)[fb]     # [E, 4]
        p = ge.pos.to(torch.float64)
        sel = sel & (p[:, 0] >= bt[:, 0]) & (p[:, 0] <= bt[:, 1]) & (p[:, 1] >= bt[:, 2]) & (p[:, 1] <= bt[:, 3])
    out = torch.nonzero(sel).reshape(-1)
    if out.numel() == 0:
        raise ValueError("WallForces: the selection holds no face (no WALL_BOUNDARY face with one incidence"
                         + (" inside the box" if boxes is not None else "") + (" among the named faces" if faces is not None else "")
                         + ")")
    return out


class WallTables:
    """What build_tables makes: bnode [Nb], wface [Nf, 4], wchunk_beg / wchunk_end [n_wchunks], gwchunk_ptr [B + 1] (int32, on the
    plan's device), faces [B] (int64, CPU: faces per graph), Nb, Nf, n_wchunks, B."""


def build_tables(plan, selected):
    """The launch tables of a selection (ascending face indices, select_faces) for a plan; plain torch ops."""
    dev = plan.es.device
    sel = torch.as_tensor(selected).reshape(-1).to(device=dev, dtype=torch.int64)
    if sel.numel() < 1:
        raise ValueError("WallForces: the selection holds no face")
    if sel.numel() > 1 and not bool((sel[1:] > sel[:-1]).all()):
        raise ValueError("build_tables: the selected faces must be ascending and unique")
    if int(sel[0]) < 0 or int(sel[-1]) >= plan.E:
        raise ValueError(f"build_tables: a face index outside 0 .. {plan.E - 1}")
    frow = plan.frow.to(torch.int64)
    if not bool(((frow[sel + 1] - frow[sel]) == 1).all()):
        raise ValueError("build_tables: every selected face needs exactly one (cell, face) incidence")
    k = plan.fk.to(torch.int64)[frow[sel]]
    s, r = plan.es.to(torch.int64)[sel], plan.er.to(torch.int64)[sel]
    bnode = torch.unique(torch.cat((s, r)))                              # (sorted)
    ja, jb = torch.searchsorted(bnode, s), torch.searchsorted(bnode, r)
    t = WallTables()
    t.bnode = bnode.to(torch.int32).contiguous()
    t.wface = torch.stack((sel, k, ja, jb), 1).to(torch.int32).contiguous()
    fb = plan.batch.to(torch.int64)[s]
    if sel.numel() > 1 and not bool((fb[1:] >= fb[:-1]).all()):
        raise ValueError("build_tables: the faces of a batch must be grouped by graph")
    B = int(plan.B)
    counts = torch.bincount(fb, minlength=B).cpu()
    cb, ce, gcp, row = [], [], [0], 0
    for b in range(B):
        n = int(counts[b])
        for st in range(row, row + n, L.WALL_FORCE_CHUNK):
            cb.append(st)
            ce.append(min(st + L.WALL_FORCE_CHUNK, row + n))
        row += n
        gcp.append(len(cb))
    t.wchunk_beg = torch.tensor(cb, dtype=torch.int32, device=dev)
    t.wchunk_end = torch.tensor(ce, dtype=torch.int32, device=dev)
    t.gwchunk_ptr = torch.tensor(gcp, dtype=torch.int32, device=dev)
    t.faces = counts.to(torch.int64)
    t.Nb, t.Nf, t.n_wchunks, t.B = int(bnode.numel()), int(sel.numel()), len(cb), B
    return t


def split_history(n, keep, hist, hist_clock):
    """The ring as the device holds it (CPU tensors: hist float64 [keep, B, 6], hist_clock int32 [keep]) -> the last
    k = min(n, keep) rows in clock order: (clock [k], rows [k, B, 6])."""
    k = min(int(n), int(keep))
    order = torch.tensor([(int(n) - k + q) % int(keep) for q in range(k)], dtype=torch.int64)
    return hist_clock[order].clone(), hist[order].clone()


class WallForces(Follower):
    KEYWORD = "wall_forces"
    NO_ANDERSON = "the ring would record forces of fields that are not steps; call gfv.wallforce.evaluate() on the converged field"

    def __init__(self, faces=None, box=None, origin=(0.0, 0.0), start=1, stride=1, stop=None, keep=4096):
        self._window = Window(start, stride, stop)
        self.keep = check_keep(keep)
        check_box(box)
        check_origin(origin)
        self._box, self._origin = box, origin         # (as given: a list is one per graph, checked against B at attach)
        if faces is not None and not isinstance(faces, torch.Tensor):
            faces = torch.as_tensor(faces)
        if faces is not None and faces.dtype not in (torch.bool, torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError(f"faces must be a bool [E] mask or an integer index tensor, got dtype {faces.dtype}")
        self._faces = faces
        # device state: allocated by attach(), never reallocated
        self.rec = self.tables = self.gb = self.partial = self.hist = self.hist_clock = self.origin = None
        self._plan = None
        self.N = 0

    start = property(lambda self: self._window.start)
    stride = property(lambda self: self._window.stride)
    stop = property(lambda self: self._window.stop)
    enabled = property(lambda self: self._window.enabled)

    # ---- the owner's side (gfv/follow.py) -------------------------------------------------------------------------------------
    _check_graphs = staticmethod(check_graphs)

    def attach(self, owner, graphs, plan, x_backup, clock, clock_word=0):
        """Called by the owner's constructor with the tensor it advances, its int32 record `clock` and the word of it that counts
        the fields written: fixes the selection, builds the tables and allocates the record and the state (once).  -> self"""
        self.check_free()
        check_graphs(graphs)
        n = check_field(x_backup)
        if n != plan.N:
            raise ValueError(f"WallForces: the node state has {n} rows, the plan {plan.N}")
        if int(plan.M) not in TERMS:
            raise ValueError(f"WallForces: the plan's reconstruction has {plan.M} terms; 2, 5, 9 and 14 are supported")
        dev = x_backup.device
        B = int(plan.B)
        origin = check_origin(self._origin, B)
        t = build_tables(plan, select_faces(graphs, self._faces, self._box))
        self.gb = torch.zeros((t.Nb, 3, 2), dtype=torch.float64, device=dev)
        self.partial = torch.zeros((t.n_wchunks, L.WALL_FORCE_SUMS), dtype=torch.float64, device=dev)
        self.hist = torch.zeros((self.keep, B, L.WALL_FORCE_SUMS), dtype=torch.float64, device=dev)
        self.hist_clock = torch.zeros(self.keep, dtype=torch.int32, device=dev)
        self.origin = torch.tensor(origin if len(origin) > 1 else origin * B, dtype=torch.float32).to(dev)
        self._xb, self._clock, self._clock_ptr = x_backup, clock, clock.data_ptr() + 4 * int(clock_word)
        self.N, self.tables, self._plan, self.rec = n, t, plan, self._window.attach(dev)
        self._claim(owner)
        return self

    def launch(self):
        """The two launches, behind the owner's advance: part of the step body (eager steps and recorded lists carry them alike)."""
        pl, t, lib, st, x_backup, clock_ptr = self._plan, self.tables, L.load(), L.stream_ptr(), self._xb, self._clock_ptr
        L.check(lib.gfv_wall_force_grad(x_backup.data_ptr(), pl.uvp_dim.data_ptr(), pl.batch.data_ptr(), pl.x_rowptr.data_ptr(),
                                        pl.x_out.data_ptr(), pl.x_B.data_ptr(), pl.An.data_ptr(), pl.rn.data_ptr(),
                                        t.bnode.data_ptr(), t.Nb, int(pl.M), clock_ptr, self.rec.data_ptr(), self.gb.data_ptr(), st),
                "gfv_wall_force_grad")
        L.check(lib.gfv_wall_force_sum(x_backup.data_ptr(), pl.uvp_dim.data_ptr(), pl.theta.data_ptr(), int(pl.theta.shape[1]),
                                       pl.pos.data_ptr(), pl.fpos.data_ptr(), pl.kS.data_ptr(), pl.es.data_ptr(), pl.er.data_ptr(),
                                       t.wface.data_ptr(), t.wchunk_beg.data_ptr(), t.wchunk_end.data_ptr(),
                                       t.gwchunk_ptr.data_ptr(), t.n_wchunks, t.Nf, t.B, self.origin.data_ptr(), self.gb.data_ptr(),
                                       clock_ptr, self.rec.data_ptr(), self.partial.data_ptr(), self.hist.data_ptr(),
                                       self.hist_clock.data_ptr(), self.keep, st), "gfv_wall_force_sum")

    def set_window(self, start=None, stride=None, stop=UNCHANGED, enabled=None):
        """`Window.set`: a new window under recorded lists.  The history so far stays: reset() starts over."""
        self._window.set(start, stride, stop, enabled)

    def reset(self):
        """`Window.reset`, in stream order; the owner's reset() calls it.  The ring needs no clearing (rows are read up to n)."""
        self._need()
        self._window.reset()

    # ---- reading (each of these is one synchronisation) ----------------------------------------------------------------------
    def count(self):
        """Samples taken so far."""
        self._need()
        return self._window.count()

    def raw(self):
        """(record [8] int32, hist [keep, B, 6] float64, hist_clock [keep] int32) as CPU copies (one synchronisation)."""
        self._need()
        nb_rec, nb_hist = 4 * L.WALL_FORCE_RECORD, 8 * self.hist.numel()
        packed = torch.cat([self.rec.view(torch.uint8), self.hist.view(torch.uint8).reshape(-1),
                            self.hist_clock.view(torch.uint8)]).cpu()
        return (packed[:nb_rec].view(torch.int32).clone(),
                packed[nb_rec:nb_rec + nb_hist].view(torch.float64).reshape(tuple(self.hist.shape)).clone(),
                packed[nb_rec + nb_hist:].view(torch.int32).clone())

    def read(self):
        """{"n", "clock" [k], "pressure" [k,B,2], "viscous" [k,B,2], "moment" [k,B,2], "faces" [B]} as CPU tensors, k = min(n, keep)
        rows in clock order (k may be 0).  pressure = (Fp_x, Fp_y), viscous = (Fv_x, Fv_y), moment = (Mp, Mv) about `origin`; the
        force of the fluid on the wall is pressure + viscous.  float64; dimensionless, in the units of the residual."""
        rec, hist, hclock = self.raw()
        n = int(rec[N_SAMPLES])
        clock, rows = split_history(n, self.keep, hist, hclock)
        return {"n": n, "clock": clock, "pressure": rows[:, :, 0:2].contiguous(), "viscous": rows[:, :, 2:4].contiguous(),
                "moment": rows[:, :, 4:6].contiguous(), "faces": self.tables.faces.clone()}

    def coefficients(self, ref_length, ref_speed=1.0):
        """{"clock" [k], "cd", "cl", "cm" [k,B]} from read(), on the host: (Fx, Fy) / (U^2 L / 2) and M / (U^2 L^2 / 2) of the total
        (pressure + viscous) force and moment, with the reference length and speed in the units of the residual."""
        return coefficients(self.read(), ref_length, ref_speed)


def coefficients(h, ref_length, ref_speed=1.0):
    for name, v in (("ref_length", ref_length), ("ref_speed", ref_speed)):
        if not _is_number(v) or not v > 0 or v == float("inf"):
            raise ValueError(f"{name} must be a positive finite number, got {v!r}")
    q = 0.5 * float(ref_speed) * float(ref_speed) * float(ref_length)
    total = h["pressure"] + h["viscous"]
    return {"clock": h["clock"], "cd": total[:, :, 0] / q, "cl": total[:, :, 1] / q,
            "cm": (h["moment"][:, :, 0] + h["moment"][:, :, 1]) / (q * float(ref_length))}


def evaluate(graphs, field, faces=None, box=None, origin=(0.0, 0.0)):
    """The forces of one field, no owner: the same two launches on a clock word of its own.  field: [N, 3] (u, v, p) or [N, 12]
    (a node state), dimensional, on the GPU.  -> [B, 6] float64 CPU tensor (Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv) per graph (one
    synchronisation)."""
    from .functions import require_gpu
    from .plan import get_plan
    if not isinstance(field, torch.Tensor) or field.dim() != 2 or field.shape[1] not in (3, 12):
        raise ValueError("evaluate: field must be a [N, 3] or [N, 12] tensor")
    require_gpu(field)
    require_gpu(graphs[0].x)
    check_graphs(graphs)
    plan = get_plan(graphs)
    if int(field.shape[0]) != plan.N:
        raise ValueError(f"evaluate: field has {int(field.shape[0])} rows, the graphs {plan.N} nodes")
    xb = torch.zeros((plan.N, 12), dtype=torch.float32, device=field.device)
    xb[:, 0:3] = field[:, 0:3].to(torch.float32)
    clock = torch.ones(1, dtype=torch.int32, device=field.device)
    wf = WallForces(faces=faces, box=box, origin=origin, start=1, keep=1).attach("evaluate", graphs, plan, xb, clock)
    wf.launch()
    rec, hist, _ = wf.raw()
    assert int(rec[N_SAMPLES]) == 1
    return hist[0]
